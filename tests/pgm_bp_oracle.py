"""numpy restatement of csrc/pgm_bp.hip: damped parallel max-product belief propagation on the binary chain with sliding-window
budgets, in the kernel's operations and their order, and the brute-force max-marginal of the budget factor that its closed form is
checked against.

The model is tests/pgm_map_oracle.py's: unary [B,N,2], pair [B,N-1,4] (row-major [x_i][x_{i+1}]), caps [B,N-h+1].  Messages are
log-ratios m(1) - m(0) in f64."""
import itertools

import numpy as np

FORCE = float(1 << 20)       # the message of a window whose cap is 0


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def budget_messages(delta, c):
    """delta [..,h] (incoming log-ratios), c [..] integer caps >= 0 -> the window's messages [..,h]: to member j, over the OTHER
    h-1 values: c > h-1: 0; c == 0: -FORCE; otherwise -max(0, the c-th largest of the others)."""
    delta = np.asarray(delta, np.float64)
    h = delta.shape[-1]
    c = np.broadcast_to(np.asarray(c, np.int64), delta.shape[:-1])
    out = np.zeros(delta.shape)
    k = np.clip(c, 1, h - 1)[..., None]
    for j in range(h):
        others = -np.sort(-np.delete(delta, j, axis=-1), axis=-1)                  # descending
        kth = np.take_along_axis(others, k - 1, axis=-1)[..., 0]
        out[..., j] = np.where(c > h - 1, 0.0, np.where(c == 0, -FORCE, -np.maximum(0.0, kth)))
    return out


def budget_messages_brute(delta, c):
    """One window: delta [h], cap c -> [h], message j = max over configurations with x_j = 1 and at most c ones of the sum of the
    others' delta where they are 1, minus the same with x_j = 0; every one of the 2^h configurations is visited.  No configuration
    with x_j = 1 (c == 0): -FORCE."""
    delta = np.asarray(delta, np.float64)
    h = len(delta)
    best = np.full((h, 2), -np.inf)
    for x in itertools.product((0, 1), repeat=h):
        if sum(x) > c:
            continue
        for j in range(h):
            v = sum(delta[m] for m in range(h) if m != j and x[m])
            best[j, x[j]] = max(best[j, x[j]], v)
    return np.where(np.isinf(best[:, 1]), -FORCE, best[:, 1] - best[:, 0])


def bp(unary, pair, caps, h, max_iter=200, damping=0.5, tol=1e-6):
    """unary [B,N,2], pair [B,N-1,4], caps [B,N-h+1] -> dict labels [B,N] int64, beliefs [B,N] f64, status [B] int32 (0 converged,
    2 a negative cap, 3 iteration cap), iters [B] int32.  Every sample iterates on its own: one that has stopped is frozen."""
    unary, pair = _f64(unary), _f64(pair)
    caps = np.asarray(caps, np.int64)
    B, N, _ = unary.shape
    W, L = N - h + 1, N - 1
    u = unary[:, :, 1] - unary[:, :, 0]
    t0, t1, t2, t3 = (pair[:, :, k] for k in range(4))
    mR, mL, mW = np.zeros((B, L)), np.zeros((B, L)), np.zeros((B, W, h))           # link i -> x_{i+1}, link i -> x_i, window w -> x_{w+j}
    infeasible = (caps < 0).any(axis=1)
    active = ~infeasible
    conv = np.zeros(B, bool)
    iters = np.zeros(B, np.int32)
    omd = 1.0 - damping

    def beliefs():
        bel = u.copy()
        bel[:, 1:] = bel[:, 1:] + mR
        bel[:, :L] = bel[:, :L] + mL
        for i in range(N):
            for w in range(max(0, i - h + 1), min(i, N - h) + 1):
                bel[:, i] = bel[:, i] + mW[:, w, i - w]
        return bel

    idx = np.arange(W)[:, None] + np.arange(h)[None, :]                            # [W,h]: the members of window w
    for _ in range(max_iter):
        if not active.any():
            break
        bel = beliefs()
        dW = bel[:, idx] - mW
        dl, dr = bel[:, :L] - mL, bel[:, 1:] - mR
        fR = np.maximum(t1, t3 + dl) - np.maximum(t0, t2 + dl)
        fL = np.maximum(t2, t3 + dr) - np.maximum(t0, t1 + dr)
        fW = budget_messages(dW, caps)
        nR, nL, nW = damping * mR + omd * fR, damping * mL + omd * fL, damping * mW + omd * fW
        change = np.maximum(np.maximum(np.abs(nR - mR).max(axis=1, initial=0.0), np.abs(nL - mL).max(axis=1, initial=0.0)),
                            np.abs(nW - mW).reshape(B, -1).max(axis=1))
        a = active
        mR[a], mL[a], mW[a] = nR[a], nL[a], nW[a]
        iters[a] += 1
        done = a & (change < tol)
        conv |= done
        active = a & ~done
    bel = np.where(infeasible[:, None], 0.0, beliefs())
    status = np.where(infeasible, 2, np.where(conv, 0, 3)).astype(np.int32)
    return {'labels': (bel > 0).astype(np.int64), 'beliefs': bel, 'status': status, 'iters': iters}
