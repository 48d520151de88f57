"""GPU: csrc/pgm_lp.hip through PgmDataPath.solve_lp against the numpy restatement (tests/pgm_lp_oracle.py), HiGHS and the exact MAP.

  * at the defaults the kernel runs the restatement's iterations: same iteration counts and status, marginals within 1e-6;
  * run long, it reaches the LP optimum HiGHS finds, which is at least the MAP objective and equals it where the LP is integral;
  * ``sample(..., lp_label=True)`` and ``write_reference_dataset(..., lp_label=True)`` carry that label as the reference's ``assign1``."""
import pickle

import numpy as np
import pytest
import torch

import pgm_lp_oracle as LO
import pgm_map_oracle as PO

pytestmark = pytest.mark.gpu

SHAPES = [(30, 9), (12, 5), (40, 13), (9, 9), (33, 2)]


def _dyadic(rng, shape, lo, hi):
    return (lo + (hi - lo) * rng.integers(0, 1 << 24, shape) / float(1 << 24)).astype(np.float32)


def _path(dev, N, h):
    from fgnn_amd import PgmDataPath
    return PgmDataPath(dev, N, h)


def _models(N, h, B, shared, seed):
    rng = np.random.default_rng(seed)
    unary = _dyadic(rng, (B, N, 2), 0, 1)
    if shared:
        pair = _dyadic(rng, (N - 1, 4), -1, 1)
        caps = rng.integers(0, h + 1, (N - h + 1,)).astype(np.int32)
        return unary, pair, caps, np.broadcast_to(pair, (B, N - 1, 4)), np.broadcast_to(caps, (B, N - h + 1))
    pair = _dyadic(rng, (B, N - 1, 4), -1, 1)
    caps = rng.integers(0, h + 1, (B, N - h + 1)).astype(np.int32)
    return unary, pair, caps, pair, caps


def _solve(path, dev, unary, pair, caps, **kw):
    lab, det = path.solve_lp(torch.from_numpy(unary).to(dev), torch.from_numpy(np.ascontiguousarray(pair)).to(dev),
                             torch.from_numpy(np.ascontiguousarray(caps)).to(dev), want_details=True, **kw)
    out = {k: v.cpu().numpy() for k, v in det.items()}
    out['labels'] = lab.cpu().numpy()
    return out


@pytest.mark.parametrize('shared', [False, True], ids=['per_sample', 'shared'])
@pytest.mark.parametrize('N,h', SHAPES)
def test_solve_lp_matches_the_numpy_admm(dev, N, h, shared):
    from fgnn_amd import _hip
    B = 384
    unary, pair, caps, pair_b, caps_b = _models(N, h, B, shared, N * 100 + h + shared)
    path = _path(dev, N, h)
    for adapt in (True, False):
        got = _solve(path, dev, unary, pair, caps, adapt=adapt)
        assert _hip.lib().fgnn_last_kernel().decode() == 'chain_budget_lp_kernel'
        assert got['labels'].dtype == np.int64 and got['marginals'].dtype == np.float64
        assert got['status'].dtype == np.int32 and got['iters'].dtype == np.int32
        want = LO.admm(unary, pair_b, caps_b, h, adapt=adapt)
        same = (got['iters'] == want['iters']) & (got['status'] == want['status'])
        print('N=%d h=%d adapt=%s: iters and status equal on %d of %d; status 3 on %d' %
              (N, h, adapt, same.sum(), B, (got['status'] == 3).sum()))
        assert same.mean() >= (0.99 if adapt else 1.0)
        assert np.abs(got['marginals'] - want['marginals'])[same].max() <= 1e-6
        assert np.abs(got['value'] - want['value'])[same].max() <= 1e-6 * (1 + np.abs(want['value'][same]).max())
        clear = same[:, None] & (np.abs(want['marginals'] - 0.5) > 1e-3)
        assert np.array_equal(got['labels'][clear], want['labels'][clear])
        assert np.array_equal(got['labels'], (got['marginals'] > 0.5).astype(np.int64))


@pytest.mark.parametrize('N,h', SHAPES)
def test_solve_lp_reaches_the_lp_optimum(dev, N, h):
    B = 64
    unary, pair, caps, _, _ = _models(N, h, B, False, 7 * N + h)
    path = _path(dev, N, h)
    got = _solve(path, dev, unary, pair, caps, max_iter=20000)
    mlab, mobj = path.solve_map(torch.from_numpy(unary).to(dev), torch.from_numpy(pair).to(dev), torch.from_numpy(caps).to(dev),
                                want_objective=True)
    mlab, mobj = mlab.cpu().numpy(), mobj.cpu().numpy()
    opt = np.array([LO.lp_highs(unary[b], pair[b], caps[b], h)[0] for b in range(B)])
    conv = got['status'] != 3
    print('N=%d h=%d: status 3 on %d of %d at 20000 iterations' % (N, h, (~conv).sum(), B))
    assert conv.any()
    assert (np.abs(got['value'] - opt) <= 1e-4 * (1 + np.abs(opt)))[conv].all()
    assert (got['value'] >= mobj - 1e-4)[conv].all()
    integral = got['status'] == 0
    assert (np.abs(got['value'] - mobj) <= 1e-4)[integral].all()
    for b in np.flatnonzero(integral[:16]):
        if N <= 14 and len(PO.brute_force(unary[b], pair[b], caps[b], h)[1]) == 1:
            assert np.array_equal(got['labels'][b], mlab[b])


@pytest.mark.parametrize('N,h', [(30, 9), (20, 4)])
def test_solve_lp_without_budgets_is_the_map(dev, N, h):
    """cap >= h everywhere: a chain is a tree, its LP is tight; converged samples are integral and give the exact MAP."""
    rng = np.random.default_rng(11)
    B = 256
    unary, pair = _dyadic(rng, (B, N, 2), 0, 1), _dyadic(rng, (B, N - 1, 4), -1, 1)
    path = _path(dev, N, h)
    u, p = torch.from_numpy(unary).to(dev), torch.from_numpy(pair).to(dev)
    lab, det = path.solve_lp(u, p, h + 1, max_iter=20000, want_details=True)
    conv = (det['status'] != 3).cpu().numpy()
    assert conv.mean() >= 0.5
    assert (det['status'].cpu().numpy()[conv] == 0).all()
    assert np.array_equal(lab.cpu().numpy()[conv], path.solve_map(u, p, h + 1).cpu().numpy()[conv])


def test_solve_lp_infeasible_shapes_and_empty(dev):
    N, h = 12, 5
    rng = np.random.default_rng(3)
    unary, pair = _dyadic(rng, (4, N, 2), 0, 1), _dyadic(rng, (4, N - 1, 4), -1, 1)
    caps = np.full((4, N - h + 1), 2, np.int32)
    caps[2, 3] = -1
    path = _path(dev, N, h)
    got = _solve(path, dev, unary, pair, caps)
    assert got['status'][2] == 2 and got['iters'][2] == 0 and got['value'][2] == -np.inf and not got['labels'][2].any()
    assert (got['status'][[0, 1, 3]] != 2).all()
    lab = path.solve_lp(torch.from_numpy(unary).to(dev), torch.from_numpy(pair).to(dev), 2)
    assert lab.shape == (4, N) and lab.dtype == torch.int64
    assert path.solve_lp(torch.zeros(0, N, 2, device=dev), torch.from_numpy(pair[0]).to(dev), 2).shape == (0, N)


@pytest.mark.parametrize('family', ['hops', 'pws', 'raw'])
def test_sample_with_lp_label(dev, family):
    N, h, B = 30, 9, 300
    path = _path(dev, N, h)
    plain = path.sample(B, family, seed=5, step=2, want_objective=True)
    out = path.sample(B, family, seed=5, step=2, want_objective=True, lp_label=True)
    assert len(out) == len(plain) + 1
    for a, b in zip(out[:-2], plain[:-1]):                                   # draws and the MAP label unchanged
        assert torch.equal(a, b)
    assert torch.equal(out[-1], plain[-1])
    lp = out[-2]
    assert lp.shape == (B, N) and lp.dtype == torch.int64
    unary, pair, _, win = PO.sample_draws(family, B, N, h, 5, 2)
    want = path.solve_lp(torch.from_numpy(unary).to(dev), torch.from_numpy(pair).to(dev), torch.from_numpy(win).to(dev))
    assert torch.equal(lp, want)
    assert torch.equal(path.sample(B, family, seed=5, step=2, lp_label=True)[-1], lp)     # order (..., assign, assign1)
    print('%s: lp label = exact label on %.3f of the variables' % (family, (lp == out[-3]).double().mean().item()))


@pytest.mark.parametrize('family', ['hops', 'raw'])
def test_write_reference_dataset_with_lp_label(dev, tmp_path, family):
    N, h, size = 30, 9, 64
    path = _path(dev, N, h)
    f = str(tmp_path / ('%s.dat' % family))
    path.write_reference_dataset(f, family, size, seed=21, batch=40, lp_label=True)
    with open(f, 'rb') as fh:
        items = [pickle.load(fh) for _ in range(size)]
        with pytest.raises(EOFError):
            pickle.load(fh)
    first = path.sample(40, family, seed=21, step=0, lp_label=True)
    second = path.sample(24, family, seed=21, step=1, lp_label=True)
    want = [torch.cat([a, b]).cpu().numpy() for a, b in zip(first, second)]
    got_lp = np.stack([it[-1] for it in items])
    assert got_lp.dtype == np.int64 and (got_lp != -1).all()
    assert np.array_equal(got_lp, want[-1])
    assert np.array_equal(np.stack([it[-2] for it in items]), want[-2])
    assert np.array_equal(np.stack([it[0] for it in items]), want[0][..., 0])
