"""numpy restatement of csrc/pgm_datapath.hip: the exact MAP of a binary chain with sliding-window budgets (same DP, same
operation order, same tie rule), brute-force enumeration to check it, and the sampler's Philox draws and model inputs.

The model: unary [N][2], pair [N-1][4] (row-major [x_i][x_{i+1}]), caps [N-h+1] (window w = x_w .. x_{w+h-1} has at most caps[w]
ones).  Arrays carry a leading batch axis here."""
import numpy as np

import fgnn_oracle as O

FAMILIES = {'raw': 0, 'pws': 1, 'hops': 2}


def _popcount(a):
    a = np.asarray(a, np.int64)
    c = np.zeros_like(a)
    while a.any():
        c += a & 1
        a = a >> 1
    return c


def chain_map(unary, pair, caps, h):
    """unary [B,N,2], pair [B,N-1,4], caps [B,N-h+1] -> (labels [B,N] int64, objective [B] f64).  State s = the last h-1 bits
    (bit 0 the newest); candidate (V[pred] + pair) + unary in f64; the dropped bit d = 1 only when strictly better; the lowest
    final state among the maxima."""
    unary = np.asarray(unary, np.float32).astype(np.float64)
    pair = np.asarray(pair, np.float32).astype(np.float64)
    caps = np.asarray(caps, np.int64)
    B, N, _ = unary.shape
    S, half = 1 << (h - 1), 1 << (h - 1) >> 1
    s = np.arange(S)
    bit, hi = s & 1, s >> 1
    pa, pb = hi, hi | half
    pc = _popcount(hi)
    V = np.full((B, S), -np.inf)
    V[:, 0], V[:, 1] = unary[:, 0, 0], unary[:, 0, 1]
    bp = np.zeros((N, B, S), bool)
    rows = np.arange(B)[:, None]
    for t in range(1, N):
        ub = unary[:, t, :][rows, bit[None, :]]
        c0 = (V[:, pa] + pair[:, t - 1, :][rows, ((pa & 1) * 2 + bit)[None, :]]) + ub
        c1 = (V[:, pb] + pair[:, t - 1, :][rows, ((pb & 1) * 2 + bit)[None, :]]) + ub
        if t >= h - 1:
            cap = caps[:, t - h + 1][:, None]
            c0 = np.where(pc[None, :] + bit[None, :] > cap, -np.inf, c0)
            c1 = np.where(pc[None, :] + 1 + bit[None, :] > cap, -np.inf, c1)
        else:
            c1 = np.full_like(c1, -np.inf)
        take = c1 > c0
        V = np.where(take, c1, c0)
        bp[t] = take
    st = np.argmax(V, axis=1)                       # first (lowest) index among the maxima
    obj = V[np.arange(B), st]
    lab = np.zeros((B, N), np.int64)
    for t in range(N - 1, 0, -1):
        lab[:, t] = st & 1
        d = bp[t, np.arange(B), st]
        st = np.where(d, half, 0) | (st >> 1)
    lab[:, 0] = st & 1
    return lab, obj


def brute_force(unary, pair, caps, h):
    """Every assignment of one instance (N <= 16): (objective, the set of optimal assignments as an [K,N] array, feasible mask,
    scores).  Scores are f64 sums; exact for dyadic potentials whatever the order."""
    unary = np.asarray(unary, np.float32).astype(np.float64)
    pair = np.asarray(pair, np.float32).astype(np.float64)
    N = unary.shape[0]
    X = (np.arange(1 << N)[:, None] >> np.arange(N)[None, :]) & 1
    score = unary[np.arange(N)[None, :], X].sum(1) + pair[np.arange(N - 1)[None, :], X[:, :-1] * 2 + X[:, 1:]].sum(1)
    ok = np.ones(len(X), bool)
    for w in range(N - h + 1):
        ok &= X[:, w:w + h].sum(1) <= caps[w]
    score = np.where(ok, score, -np.inf)
    best = score.max()
    return best, X[score == best], ok, score


def feasible(labels, caps, h):
    """[B] bool: every window budget holds."""
    labels = np.asarray(labels)
    N = labels.shape[1]
    return np.all([labels[:, w:w + h].sum(1) <= np.asarray(caps)[:, w] for w in range(N - h + 1)], axis=0)


def philox_words(B, nwords, seed, offset):
    """[B, nwords] uint32: word w of sample b = philox(counter (b, w >> 2, offset lo, offset hi), key (seed lo, seed hi))[w & 3]."""
    nq = (nwords + 3) // 4
    b = np.repeat(np.arange(B, dtype=np.uint64), nq)
    q = np.tile(np.arange(nq, dtype=np.uint64), B)
    ctr = np.stack([b, q, np.full_like(b, offset & 0xFFFFFFFF), np.full_like(b, (offset >> 32) & 0xFFFFFFFF)], axis=-1)
    r = O.philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return r.reshape(B, nq * 4)[:, :nwords]


def sample_draws(family, B, N, h, seed, offset, cap=5, transition=(0, .1, .2, 1)):
    """The sampler's models: (unary [B,N,2] f32, pair [B,N-1,4] f32, position caps [B,N] int64 (hops) or None, window caps
    [B,N-h+1] int64)."""
    fam = FAMILIES[family]
    nw = 2 * N + (N - 1 if fam else 0) + (N if fam == 2 else 0)
    r = philox_words(B, nw, seed, offset)
    u = (r >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    unary = u[:, :2 * N].reshape(B, N, 2)
    pair = np.zeros((B, N - 1, 4), np.float32)
    if fam == 0:
        pair[:] = np.asarray(transition, np.float32)
    else:
        pair[:, :, 3] = np.float32(2) * u[:, 2 * N:3 * N - 1]
    if fam == 2:
        pos = 1 + ((r[:, 3 * N - 1:4 * N - 1].astype(np.uint64) * np.uint64(h - 1)) >> np.uint64(32)).astype(np.int64)
        win = pos[:, h // 2:h // 2 + N - h + 1]
    else:
        pos, win = None, np.full((B, N - h + 1), cap, np.int64)
    return unary, pair, pos, win


def features(unary, pair, pos, h):
    """Model inputs as the sampler writes them: node [B,2,N,1], pws [B,4,N,1], hops [B,h,N,1] (None without position caps)."""
    B, N, _ = unary.shape
    node = np.ascontiguousarray(unary.transpose(0, 2, 1))[..., None]
    pws = np.zeros((B, 4, N), np.float32)
    pws[:, :, :N - 1] = pair.transpose(0, 2, 1)
    hops = None
    if pos is not None:
        hot = np.full((B, N), h - 1, np.int64)
        hot[:, h // 2:N - h // 2] = pos[:, h // 2:N - h // 2]
        hops = (np.arange(h)[None, :, None] == hot[:, None, :]).astype(np.float32)[..., None]
    return node, pws[..., None], hops
