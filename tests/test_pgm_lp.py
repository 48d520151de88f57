"""CPU: the LP-relaxation solver's checker and host side (csrc/pgm_lp.hip, fgnn_amd/pgm_datapath.py: solve_lp).

  * the two closed-form factor QPs of tests/pgm_lp_oracle.py against brute force;
  * the numpy ADMM (which the GPU tests hold the kernel to) reaches the LP optimum HiGHS finds, which bounds the exact MAP from above,
    and is tight on chains without budgets;
  * argument validation happens before any launch, so it is testable without a device;
  * the kernel keeps everything in registers and LDS (compiler resource report, cross-compiled for gfx950)."""
import ctypes
import os

import numpy as np
import pytest

import pgm_lp_oracle as LO
import pgm_map_oracle as PO

N, H = 30, 9
EINVAL = -1                                    # FGNN_EINVAL


def _dyadic(rng, shape, lo, hi):
    return (lo + (hi - lo) * rng.integers(0, 1 << 24, shape) / float(1 << 24)).astype(np.float32)


def test_link_factor_qp_against_a_grid():
    """The closed form is feasible and at least as good as every point of a fine grid over (z1, z2), with y eliminated exactly
    (k >= 0: y = min(z1, z2); k < 0: y = max(0, z1 + z2 - 1))."""
    rng = np.random.default_rng(1)
    g = np.linspace(0, 1, 401)
    Z1, Z2 = np.meshgrid(g, g, indexing='ij')
    for _ in range(300):
        c1, c2 = rng.uniform(-1.5, 2.5, 2)
        k = rng.choice([0.0, rng.uniform(-3, 3)])
        z1, z2, y = (float(v) for v in LO.link_qp(c1, c2, k))
        assert 0 <= z1 <= 1 and 0 <= z2 <= 1 and max(0.0, z1 + z2 - 1) - 1e-15 <= y <= min(z1, z2) + 1e-15
        F = lambda a, b, yy: 0.5 * (a - c1) ** 2 + 0.5 * (b - c2) ** 2 - k * yy
        Yg = np.minimum(Z1, Z2) if k >= 0 else np.maximum(0.0, Z1 + Z2 - 1)
        grid = F(Z1, Z2, Yg)
        best = grid.min()
        assert F(z1, z2, y) <= best + 1e-12, (c1, c2, k)
        # strictly convex in (z1, z2): the grid's argmin lies next to the closed form
        i, j = np.unravel_index(np.argmin(grid), grid.shape)
        assert abs(g[i] - z1) <= 0.01 and abs(g[j] - z2) <= 0.01, (c1, c2, k, z1, z2, g[i], g[j])


def test_budget_projection_against_bisection():
    rng = np.random.default_rng(2)
    for _ in range(400):
        h = int(rng.integers(2, 14))
        b = int(rng.integers(0, h))
        c = rng.uniform(-1, 2, h)
        if rng.random() < 0.2:
            c[rng.integers(0, h, 3)] = c[0]                                  # repeated breakpoints
        z = LO.budget_projection(c[None], np.array([b]))[0]
        clip = np.clip(c, 0, 1)
        if clip.sum() <= b:
            want = clip
        else:
            lo, hi = 0.0, float(c.max()) + 1
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                lo, hi = (mid, hi) if np.clip(c - mid, 0, 1).sum() > b else (lo, mid)
            want = np.clip(c - 0.5 * (lo + hi), 0, 1)
        assert np.abs(z - want).max() <= 1e-9, (c, b, z, want)
        assert (z >= 0).all() and (z <= 1).all() and z.sum() <= b + 1e-9


_RUNS = {}


def _family_run(family):
    """~50 reference models of `family`: the numpy ADMM at 20000 iterations, HiGHS and the exact MAP (computed once)."""
    if family not in _RUNS:
        B = 48
        unary, pair, _, win = PO.sample_draws(family, B, N, H, seed=7, offset=0)
        r = LO.admm(unary, pair, win, H, max_iter=20000)
        opt = np.array([LO.lp_highs(unary[b], pair[b], win[b], H)[0] for b in range(B)])
        _, mobj = PO.chain_map(unary, pair, win, H)
        _RUNS[family] = (r, opt, mobj)
    return _RUNS[family]


@pytest.mark.parametrize('family', ['hops', 'pws', 'raw'])
def test_numpy_admm_reaches_the_highs_optimum(family):
    r, opt, mobj = _family_run(family)
    conv = r['status'] != 3
    print('%s: %d of %d converged within 20000 iterations' % (family, conv.sum(), len(conv)))
    assert conv.any()
    assert (np.abs(r['value'] - opt) <= 1e-4 * (1 + np.abs(opt)))[conv].all(), (r['value'] - opt)[conv]
    assert (opt >= mobj - 1e-9).all()                                          # the relaxation bounds the MAP from above
    assert (r['value'] >= mobj - 1e-4)[conv].all()
    assert (r['status'][conv] <= 1).all()
    z = r['marginals']
    assert (z >= 0).all() and (z <= 1).all()


def test_chain_lp_without_budgets_is_tight():
    """cap >= h leaves a chain, a tree: its LP optimum is the MAP (unique for these potentials), so converged samples give it."""
    rng = np.random.default_rng(3)
    B, n, h = 48, 20, 5
    unary, pair = _dyadic(rng, (B, n, 2), 0, 1), _dyadic(rng, (B, n - 1, 4), -1, 1)
    caps = np.full((B, n - h + 1), h)
    r = LO.admm(unary, pair, caps, h, max_iter=20000)
    lab, mobj = PO.chain_map(unary, pair, caps, h)
    conv = r['status'] != 3
    print('no budgets: %d of %d converged' % (conv.sum(), B))
    assert conv.sum() >= B // 2
    assert np.array_equal(r['labels'][conv], lab[conv])
    assert (r['status'][conv] == 0).all()
    assert np.allclose(r['value'][conv], mobj[conv], atol=1e-4)


def test_oracle_infeasible_and_iteration_cap():
    rng = np.random.default_rng(4)
    unary, pair = _dyadic(rng, (3, 12, 2), 0, 1), _dyadic(rng, (3, 11, 4), -1, 1)
    caps = np.full((3, 8), 2)
    caps[1, 4] = -1
    r = LO.admm(unary, pair, caps, 5, max_iter=3)
    assert list(r['status']) == [3, 2, 3] and list(r['iters']) == [3, 0, 3]
    assert r['value'][1] == -np.inf and not r['labels'][1].any()
    r0 = LO.admm(unary, pair, caps, 5, max_iter=0)
    assert (r0['marginals'][[0, 2]] == 0.5).all() and not r0['labels'].any()   # the start: z = 1/2, ties to state 0


def test_library_lp_footprint_and_validation_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    assert L.fgnn_abi_version() == _hip.ABI_VERSION == 15
    q = lambda n, h: int(L.fgnn_chain_budget_lp_lds_bytes(n, h))
    W = N - H + 1
    assert q(N, H) == (8 * (4 * N + 5 * (N - 1) + 2 * W * H) + 4 * (2 * N + 4 * (N - 1)) + 4 * (2 * W + 1) + 15) // 16 * 16
    for n, h in ((30, 14), (30, 1), (8, 9)):
        assert q(n, h) == -1
    assert b'outside 2..13' in (L.fgnn_chain_budget_lp_lds_bytes(30, 14), L.fgnn_last_error())[1]
    assert q(2000, 13) == -1 and b'LDS' in L.fgnn_last_error()
    one = ctypes.c_void_p(16)                      # a non-NULL pointer that is never dereferenced on these paths
    lp = lambda u=one, B=4, n=N, h=H, it=1000, tol=1e-6, eta=0.1, lab=one: L.fgnn_chain_budget_lp(
        u, 2 * n, one, 0, one, 0, B, n, h, it, tol, eta, 1, lab, None, None, None, None, None)
    assert lp(h=14) == _hip.EUNSUPPORTED and lp(n=8) == _hip.EUNSUPPORTED
    assert lp(u=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert lp(lab=None) == EINVAL
    assert lp(it=-1) == EINVAL and b'max_iter' in L.fgnn_last_error()
    assert lp(tol=float('nan')) == EINVAL and lp(tol=-1.0) == EINVAL and b'tol' in L.fgnn_last_error()
    assert lp(eta=0.0) == EINVAL and lp(eta=float('inf')) == EINVAL and b'eta' in L.fgnn_last_error()
    assert lp(B=-1) == EINVAL
    assert lp(u=None, lab=None, B=0) == 0                               # empty batch: nothing to do


def test_solve_lp_validates_on_the_host():
    import torch
    from fgnn_amd import PgmDataPath
    path = PgmDataPath.__new__(PgmDataPath)                                   # host side only: no device is touched
    path.N, path.h, path.device = N, H, torch.device('cuda:0')
    u, p, c = torch.zeros(2, N, 2), torch.zeros(N - 1, 4), 3
    for kw, what in (({'max_iter': -1}, 'max_iter'), ({'tol': float('nan')}, 'tol'), ({'eta': 0}, 'eta'),
                     ({'eta': float('inf')}, 'eta')):
        with pytest.raises(ValueError, match=what):
            path.solve_lp(u, p, c, **kw)
    with pytest.raises(ValueError, match='unary'):
        path.solve_lp(torch.zeros(2, N, 3), p, c)


@pytest.mark.skipif(not os.path.exists(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')), reason='no hipcc')
def test_lp_kernel_has_no_scratch():
    from scratch_report import scratch
    rep = scratch('pgm_lp.hip')
    hits = {k: v for k, v in rep.items() if 'chain_budget_lp_kernel' in k}
    assert len(hits) == 1, rep
    assert not any(hits.values()), hits
