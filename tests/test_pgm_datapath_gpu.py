"""GPU: csrc/pgm_datapath.hip through PgmDataPath against the numpy restatement (tests/pgm_map_oracle.py).

  * ``solve_map``: labels and objective bit for bit equal to the numpy DP (same order of operations, same ties) on dyadic
    potentials, every window budget met, brute force where N <= 14, cap >= h the unconstrained Viterbi;
  * ``sample``: the Philox draws, the model inputs in the reference's layouts and the labels, each family;
  * ``write_reference_dataset``: the reference's pickle stream, read back as RandomPGMData reads it."""
import pickle

import numpy as np
import pytest
import torch

import pgm_map_oracle as PO

pytestmark = pytest.mark.gpu


def _dyadic(rng, shape, lo, hi):
    return (lo + (hi - lo) * rng.integers(0, 1 << 24, shape) / float(1 << 24)).astype(np.float32)


def _path(dev, N, h):
    from fgnn_amd import PgmDataPath
    return PgmDataPath(dev, N, h)


@pytest.mark.parametrize('N,h,B', [(30, 9, 4096), (12, 5, 1000), (16, 3, 1000), (40, 13, 130), (33, 2, 1000), (9, 9, 77)])
def test_solve_map_matches_the_numpy_dp(dev, N, h, B):
    from fgnn_amd import _hip
    rng = np.random.default_rng(N * 100 + h)
    unary = _dyadic(rng, (B, N, 2), 0, 1)
    pair = _dyadic(rng, (B, N - 1, 4), -1, 1)
    caps = rng.integers(0, h + 1, (B, N - h + 1)).astype(np.int32)
    path = _path(dev, N, h)
    lab, obj = path.solve_map(torch.from_numpy(unary).to(dev), torch.from_numpy(pair).to(dev), torch.from_numpy(caps).to(dev),
                              want_objective=True)
    assert _hip.lib().fgnn_last_kernel().decode() == 'chain_budget_map_kernel'
    lab, obj = lab.cpu().numpy(), obj.cpu().numpy()
    want_lab, want_obj = PO.chain_map(unary, pair, caps, h)
    assert lab.dtype == np.int64 and obj.dtype == np.float64
    assert np.array_equal(obj, want_obj)
    assert np.array_equal(lab, want_lab)
    assert PO.feasible(lab, caps, h).all()
    if N <= 14:
        for b in range(64):
            best, argmaxes, _, _ = PO.brute_force(unary[b], pair[b], caps[b], h)
            assert obj[b] == best
            if len(argmaxes) == 1:
                assert np.array_equal(lab[b], argmaxes[0])


@pytest.mark.parametrize('N,h', [(30, 9), (20, 4)])
def test_solve_map_shared_inputs_and_no_budget(dev, N, h):
    """pair and caps shared by the batch (batch stride 0); cap >= h is the unconstrained Viterbi (h = 2 with no budget)."""
    rng = np.random.default_rng(5)
    B = 500
    unary = _dyadic(rng, (B, N, 2), 0, 1)
    pair = _dyadic(rng, (N - 1, 4), -1, 1)
    path = _path(dev, N, h)
    for cap in (3, h, h + 4):
        lab, obj = path.solve_map(torch.from_numpy(unary).to(dev), torch.from_numpy(pair).to(dev), cap, want_objective=True)
        want_lab, want_obj = PO.chain_map(unary, np.broadcast_to(pair, (B, N - 1, 4)), np.full((B, N - h + 1), cap), h)
        assert np.array_equal(lab.cpu().numpy(), want_lab) and np.array_equal(obj.cpu().numpy(), want_obj)
        if cap >= h:
            v_lab, v_obj = PO.chain_map(unary, np.broadcast_to(pair, (B, N - 1, 4)), np.full((B, N - 1), 2), 2)
            assert np.array_equal(lab.cpu().numpy(), v_lab) and np.array_equal(obj.cpu().numpy(), v_obj)
    # a [N-1, 2, 2] table is the same row-major [x_i][x_{i+1}] table
    lab2 = path.solve_map(torch.from_numpy(unary).to(dev), torch.from_numpy(pair).reshape(N - 1, 2, 2).to(dev), 3)
    assert torch.equal(lab2.cpu(), torch.from_numpy(PO.chain_map(unary, np.broadcast_to(pair, (B, N - 1, 4)),
                                                                 np.full((B, N - h + 1), 3), h)[0]))
    assert path.solve_map(torch.zeros(0, N, 2, device=dev), torch.from_numpy(pair).to(dev), 3).shape == (0, N)


def _check_sample(dev, family, B, N, h, seed, step, cap=5):
    path = _path(dev, N, h)
    out = path.sample(B, family, seed=seed, step=step, cap=cap, want_objective=True)
    assert len(out) == {'hops': 5, 'pws': 4, 'raw': 3}[family]
    node, label, obj = out[0], out[-2], out[-1]
    unary, pair, pos, win = PO.sample_draws(family, B, N, h, seed, step, cap=cap)
    w_node, w_pws, w_hops = PO.features(unary, pair, pos, h)
    assert node.shape == (B, 2, N, 1) and node.dtype == torch.float32
    assert np.array_equal(node.cpu().numpy(), w_node)                         # the draws, bit for bit
    if family != 'raw':
        pws = out[1].cpu().numpy()
        assert pws.shape == (B, 4, N, 1) and np.array_equal(pws, w_pws)
        assert not pws[:, :3].any() and not pws[:, :, N - 1].any()           # only the [1][1] slot, zero at the last position
    if family == 'hops':
        hops = out[2].cpu().numpy()
        assert hops.shape == (B, h, N, 1) and np.array_equal(hops, w_hops)
        assert (hops.sum(1) == 1).all()                                       # one-hot ...
        border = list(range(h // 2)) + list(range(N - h // 2, N))
        assert (hops[:, h - 1, border] == 1).all()                            # ... h-1 at the borders
    want_lab, want_obj = PO.chain_map(unary, pair, win, h)
    assert label.dtype == torch.int64 and np.array_equal(label.cpu().numpy(), want_lab)
    assert np.array_equal(obj.cpu().numpy(), want_obj)
    assert PO.feasible(want_lab, win, h).all()
    return out, unary, pair, pos


@pytest.mark.parametrize('family', ['hops', 'pws', 'raw'])
def test_sample_matches_the_restatement(dev, family):
    _check_sample(dev, family, 1021, 30, 9, seed=11, step=3)


def test_sample_other_shapes(dev):
    _check_sample(dev, 'hops', 200, 17, 4, seed=2, step=0)
    _check_sample(dev, 'pws', 200, 40, 13, seed=2, step=1, cap=7)
    _check_sample(dev, 'raw', 200, 30, 9, seed=2, step=1, cap=9)             # cap >= h: RandomPGMNoHop


def test_sample_is_a_function_of_seed_and_step(dev):
    path = _path(dev, 30, 9)
    a, b = path.sample(512, 'hops', seed=4, step=9), path.sample(512, 'hops', seed=4, step=9)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = path.sample(512, 'hops', seed=4, step=10)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1]) and not torch.equal(a[2], c[2])
    d = path.sample(100, 'hops', seed=4, step=9)                                # batch size does not change an item
    assert all(torch.equal(x[:100], y) for x, y in zip(a, d))


def test_sample_distributions(dev):
    B, N, h = 4096, 30, 9
    node, pws, hops, label = _path(dev, N, h).sample(B, 'hops', seed=1, step=0)
    u = node.cpu().numpy()
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 0.01
    bonus = pws[:, 3, :N - 1].cpu().numpy()
    assert bonus.min() >= 0 and bonus.max() < 2 and abs(bonus.mean() - 1.0) < 0.02
    caps = hops[:, :, h // 2:N - h // 2, 0].argmax(1).cpu().numpy()
    freq = np.bincount(caps.ravel(), minlength=h) / caps.size
    assert freq[0] == 0 and np.all(np.abs(freq[1:h] - 1.0 / (h - 1)) < 0.1 / (h - 1))
    # the exact labels are not the unary argmax: the budgets and link bonuses move a good share of them
    lab = label.cpu().numpy()
    agree = ((u[:, 1, :, 0] > u[:, 0, :, 0]) == lab).mean()
    assert 0.5 < agree < 0.98


@pytest.mark.parametrize('family', ['hops', 'pws', 'raw'])
def test_write_reference_dataset_round_trip(dev, tmp_path, family):
    N, h, size = 30, 9, 64
    path = _path(dev, N, h)
    f = str(tmp_path / ('%s.dat' % family))
    path.write_reference_dataset(f, family, size, seed=21, batch=40)
    items = []
    with open(f, 'rb') as fh:                                                   # lib/data/random_pgm_data.py:11-15
        for _ in range(size):
            items.append(pickle.load(fh))
        with pytest.raises(EOFError):
            pickle.load(fh)
    arity = {'hops': 5, 'pws': 4, 'raw': 3}[family]
    shapes = {'hops': [(2, N), (4, N, 1), (h, N, 1), (N,), (N,)], 'pws': [(2, N), (4, N, 1), (N,), (N,)], 'raw': [(2, N), (N,), (N,)]}
    for it in items:
        assert isinstance(it, tuple) and len(it) == arity
        assert [a.shape for a in it] == shapes[family]
        assert all(a.dtype == np.float32 for a in it[:-2]) and it[-2].dtype == np.int64 and it[-1].dtype == np.int64
        assert (it[-1] == -1).all()                                              # no LP-relaxation label
    first, second = path.sample(40, family, seed=21, step=0), path.sample(24, family, seed=21, step=1)
    want = [torch.cat([a, b]).cpu().numpy() for a, b in zip(first, second)]
    got_lab = np.stack([it[-2] for it in items])
    assert np.array_equal(got_lab, want[-1])
    assert np.array_equal(np.stack([it[0] for it in items]), want[0][..., 0])
    for k in range(1, arity - 2):
        assert np.array_equal(np.stack([it[k] for it in items]), want[k])
