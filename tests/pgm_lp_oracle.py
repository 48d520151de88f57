"""numpy restatement of csrc/pgm_lp.hip: the LP relaxation of the binary chain with sliding-window budgets, solved by the kernel's
ADMM (same factors, same order of operations, same stopping and step-size rules), and the same LP handed to HiGHS.

The model is tests/pgm_map_oracle.py's: unary [B,N,2], pair [B,N-1,4] (row-major [x_i][x_{i+1}]), caps [B,N-h+1].  The LP, in
binary form: z_i = mu_i(1) in [0,1], y_i = mu_{i,i+1}(1,1) with max(0, z_i + z_{i+1} - 1) <= y_i <= min(z_i, z_{i+1}), and
sum_{j=w}^{w+h-1} z_j <= caps[w] for every window with caps[w] < h; maximise the expected log-potential sum."""
import numpy as np

INTEGRAL_EPS = 1e-6          # status 0: every z_i within this of 0 or 1
ADAPT_EVERY = 50             # adapt: residual balancing after every 50th iteration


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def link_coefficients(pair):
    """pair [..,4] -> (constant, coefficient of z_i, of z_{i+1}, of y_i) of the link's expected log-potential."""
    p = _f64(pair)
    return p[..., 0], p[..., 2] - p[..., 0], p[..., 1] - p[..., 0], ((p[..., 0] - p[..., 1]) - p[..., 2]) + p[..., 3]


def link_qp(c1, c2, k):
    """argmin 1/2 (z1 - c1)^2 + 1/2 (z2 - c2)^2 - k y over the 2x2 marginal polytope (z in [0,1]^2, max(0, z1 + z2 - 1) <= y <=
    min(z1, z2)).  k >= 0: y = min(z1, z2) and three cases; k < 0: flip z2 -> 1 - z2 (then y -> z1 - y)."""
    c1, c2, k = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (c1, c2, k)))
    neg = k < 0
    a = np.where(neg, c1 + k, c1)
    b = np.where(neg, 1.0 - c2, c2)
    kk = np.where(neg, -k, k)
    clip = lambda v: np.minimum(np.maximum(v, 0.0), 1.0)
    mid = clip(((a + b) + kk) * 0.5)
    first = a >= b + kk
    second = ~first & (b >= a + kk)
    z1 = np.where(first, clip(a), np.where(second, clip(a + kk), mid))
    z2 = np.where(first, clip(b + kk), np.where(second, clip(b), mid))
    y = np.minimum(z1, z2)
    return z1, np.where(neg, 1.0 - z2, z2), np.where(neg, z1 - y, y)


def budget_projection(c, b):
    """Euclidean projection of c [..,h] onto {0 <= z <= 1, sum z <= b} (b [..] integers >= 0).  Clip; if the sum is over b, tau >= 0
    solves sum clip(c - tau, 0, 1) = b: t_lo = the largest of 0 and the breakpoints c_j, c_j - 1 where that sum is still > b; on
    (t_lo, next breakpoint) the sum is linear, ones = {c_j - 1 > t_lo}, free = {c_j - 1 <= t_lo < c_j}, tau = (|ones| + sum_free
    c_j - b) / |free|.  Every sum runs over j in order."""
    c = np.asarray(c, np.float64)
    h = c.shape[-1]
    b = np.asarray(b, np.float64)
    clip = lambda v: np.minimum(np.maximum(v, 0.0), 1.0)
    s = np.zeros(c.shape[:-1])
    for j in range(h):
        s = s + clip(c[..., j])
    over = s > b
    cand = np.concatenate([c, c - 1.0], axis=-1)                       # candidate j -> c_j, h + j -> c_j - 1
    g = np.zeros(cand.shape)
    for j in range(h):
        g = g + clip(c[..., j:j + 1] - cand)
    tlo = np.max(np.where(g > b[..., None], cand, 0.0), axis=-1)
    tlo = np.maximum(tlo, 0.0)
    acc = np.zeros(c.shape[:-1])
    nf = np.zeros(c.shape[:-1])
    for j in range(h):
        one = c[..., j] - 1.0 > tlo
        free = ~one & (c[..., j] > tlo)
        acc = np.where(one, acc + 1.0, np.where(free, acc + c[..., j], acc))
        nf = nf + free
    tau = np.where(nf > 0, (acc - b) / np.maximum(nf, 1), tlo)
    return np.where(over[..., None], clip(c - tau[..., None]), clip(c))


def admm(unary, pair, caps, h, max_iter=1000, tol=1e-6, eta=0.1, adapt=True):
    """The kernel's ADMM on B chains -> dict(labels [B,N] int64, marginals [B,N], value [B], status [B] int32, iters [B] int32).

    Start z = 1/2, lambda = 0.  Variable i's unary (u_i(1) - u_i(0)) is shared equally by its deg_i factors.  Per iteration:
    every factor solves its QP around c = z + (share + own linear term + lambda) / eta; z_new = (sum of the copies) / deg_i, summed
    left link, right link, then the budget windows in order; lambda -= eta (q - z_new).  Residuals over the S = 2(N-1) + h nb
    variable-factor slots: primal P = sum (q - z_new)^2, dual D = sum deg_i (z_new - z)^2; stop when P / S < tol^2 and D / S <
    tol^2 (both RMS residuals below tol).  adapt: after every ADAPT_EVERY-th iteration, eta *= 2 when P > 100 D, eta /= 2 when
    D > 100 P (RMS ratio 10)."""
    u, p = _f64(unary), _f64(pair)
    caps = np.asarray(caps, np.int64)
    B, N, _ = u.shape
    W = N - h + 1
    p = np.broadcast_to(p, (B, N - 1, 4))
    caps = np.broadcast_to(caps, (B, W))
    act = caps < h
    infeasible = (caps < 0).any(1)
    deg = np.zeros((B, N))
    deg[:, 1:] += 1
    deg[:, :-1] += 1
    for w in range(W):
        deg[:, w:w + h] += act[:, w:w + 1]
    theta = u[:, :, 1] - u[:, :, 0]
    share = theta / deg
    p0, a1, a2, c12 = link_coefficients(p)
    nslots = 2.0 * (N - 1) + h * act.sum(1)
    bcap = np.where(act, caps, h).astype(np.float64)
    win = np.arange(W)[:, None] + np.arange(h)[None, :]                  # [W, h] variable of slot (w, j)

    z = np.full((B, N), 0.5)
    lamL = np.zeros((B, N - 1, 2))
    lamB = np.zeros((B, W, h))
    y = np.zeros((B, N - 1))
    et = np.full(B, float(eta))
    run = ~infeasible
    conv = np.zeros(B, bool)
    iters = np.zeros(B, np.int32)
    tol2 = float(tol) * float(tol)
    for _ in range(int(max_iter)):
        if not run.any():
            break
        e = et[:, None]
        c1 = z[:, :-1] + ((share[:, :-1] + a1) + lamL[..., 0]) / e
        c2 = z[:, 1:] + ((share[:, 1:] + a2) + lamL[..., 1]) / e
        q1, q2, qy = link_qp(c1, c2, c12 / e)
        cb = z[:, win] + (share[:, win] + lamB) / e[..., None]
        qb = budget_projection(cb, bcap)
        s = np.zeros((B, N))
        s[:, 1:] = q2
        s[:, 0] = q1[:, 0]
        s[:, 1:-1] = s[:, 1:-1] + q1[:, 1:]
        for w in range(W):
            s[:, w:w + h] = np.where(act[:, w:w + 1], s[:, w:w + h] + qb[:, w], s[:, w:w + h])
        zn = s / deg
        dL1, dL2 = q1 - zn[:, :-1], q2 - zn[:, 1:]
        dB = qb - zn[:, win]
        r = run[:, None]
        lamL = np.where(r[..., None], lamL - e[..., None] * np.stack([dL1, dL2], -1), lamL)
        lamB = np.where(r[..., None] & act[..., None], lamB - e[..., None] * dB, lamB)
        P = (dL1 * dL1).sum(1) + (dL2 * dL2).sum(1) + np.where(act[..., None], dB * dB, 0.0).sum((1, 2))
        D = (deg * (zn - z) * (zn - z)).sum(1)
        y = np.where(r, qy, y)
        z = np.where(r, zn, z)
        iters = iters + run
        done = run & (P / nslots < tol2) & (D / nslots < tol2)
        conv |= done
        if adapt:
            chk = run & ~done & (iters % ADAPT_EVERY == 0)
            up = chk & (P > 100.0 * D)
            down = chk & ~up & (D > 100.0 * P)
            et = np.where(up, et * 2.0, np.where(down, et * 0.5, et))
        run = run & ~done
    return finish(u, p, z, y, infeasible, conv, iters)


def finish(u, p, z, y, infeasible, conv, iters):
    """Outputs from the last iterate: y clipped into its link bounds; the objective summed variable by variable, then link by link."""
    B, N, _ = u.shape
    zl, zr = z[:, :-1], z[:, 1:]
    y = np.minimum(np.maximum(y, np.maximum(0.0, (zl + zr) - 1.0)), np.minimum(zl, zr))
    p0, a1, a2, c12 = link_coefficients(p)
    v = np.zeros(B)
    for i in range(N):
        v = v + (u[:, i, 0] + (u[:, i, 1] - u[:, i, 0]) * z[:, i])
    for i in range(N - 1):
        v = v + (((p0[:, i] + a1[:, i] * zl[:, i]) + a2[:, i] * zr[:, i]) + c12[:, i] * y[:, i])
    integral = (np.minimum(z, 1.0 - z) <= INTEGRAL_EPS).all(1)
    status = np.where(infeasible, 2, np.where(~conv, 3, np.where(integral, 0, 1))).astype(np.int32)
    z = np.where(infeasible[:, None], 0.0, z)
    v = np.where(infeasible, -np.inf, v)
    return dict(labels=(z > 0.5).astype(np.int64), marginals=z, value=v, status=status, iters=iters.astype(np.int32))


def lp_highs(unary, pair, caps, h):
    """The same LP for scipy.optimize.linprog(method='highs'), one instance: (optimum, z [N]) or (-inf, None) when infeasible."""
    from scipy.optimize import linprog
    u, p = _f64(unary), _f64(pair)
    caps = np.asarray(caps, np.int64)
    N = u.shape[0]
    if (caps < 0).any():
        return -np.inf, None
    p0, a1, a2, c12 = link_coefficients(p)
    nv = 2 * N - 1                                                      # z_0 .. z_{N-1}, y_0 .. y_{N-2}
    cost = np.zeros(nv)
    cost[:N] = u[:, 1] - u[:, 0]
    cost[:N - 1] += a1
    cost[1:N] += a2
    cost[N:] = c12
    const = u[:, 0].sum() + p0.sum()
    rows, rhs = [], []
    for i in range(N - 1):
        for coef, b in (({N + i: 1, i: -1}, 0), ({N + i: 1, i + 1: -1}, 0), ({i: 1, i + 1: 1, N + i: -1}, 1)):
            r = np.zeros(nv)
            for k, v in coef.items():
                r[k] = v
            rows.append(r)
            rhs.append(b)
    for w in range(N - h + 1):
        if caps[w] < h:
            r = np.zeros(nv)
            r[w:w + h] = 1
            rows.append(r)
            rhs.append(caps[w])
    res = linprog(-cost, A_ub=np.array(rows), b_ub=np.array(rhs, np.float64), bounds=[(0, 1)] * nv, method='highs')
    assert res.status == 0, res.message
    return const - res.fun, res.x[:N]
