"""GPU: csrc/pgm_bp.hip through PgmDataPath.solve_bp against the numpy restatement (tests/pgm_bp_oracle.py) and the exact solver.

  * on dyadic potentials every quantity of the undamped run, and of a run of 16 halvings, is an exact f64 value whatever the order
    of the sums: beliefs, labels and iteration counts equal the restatement's bit for bit, on every sample;
  * at another damping the beliefs agree within 1e-9, at the defaults the runs stop in the same iteration;
  * without budgets max-product is exact: ``solve_bp`` equals ``solve_map``;
  * ``sample(..., bp_label=True)`` and ``evaluate(..., bp=True)`` carry and score that label."""
import numpy as np
import pytest
import torch

import pgm_bp_oracle as BO

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (9, 2), (12, 4), (13, 13), (30, 9), (30, 13)]
B = 67                                           # not a multiple of any workgroup's wave count
cases = pytest.mark.parametrize('shared', [False, True], ids=['per_sample', 'shared'])
shapes = pytest.mark.parametrize('N,h', SHAPES)


def _dyadic(rng, shape, lo, hi):
    return (lo + (hi - lo) * rng.integers(0, 1 << 24, shape) / float(1 << 24)).astype(np.float32)


def _path(dev, N, h):
    from fgnn_amd import PgmDataPath
    return PgmDataPath(dev, N, h)


_MODELS, _WANT = {}, {}


def _models(N, h, shared, cap_lo=0):
    """(unary, pair, caps as passed, pair and caps with the batch axis) of the case; caps drawn from cap_lo .. h."""
    key = (N, h, shared, cap_lo)
    if key not in _MODELS:
        rng = np.random.default_rng(1000 * N + 10 * h + shared)
        unary = _dyadic(rng, (B, N, 2), 0, 1)
        if shared:
            pair = _dyadic(rng, (N - 1, 4), -1, 1)
            caps = rng.integers(cap_lo, h + 1, (N - h + 1,)).astype(np.int32)
            _MODELS[key] = (unary, pair, caps, np.broadcast_to(pair, (B, N - 1, 4)), np.broadcast_to(caps, (B, N - h + 1)))
        else:
            pair = _dyadic(rng, (B, N - 1, 4), -1, 1)
            caps = rng.integers(cap_lo, h + 1, (B, N - h + 1)).astype(np.int32)
            _MODELS[key] = (unary, pair, caps, pair, caps)
    return _MODELS[key]


def _want(N, h, shared, cap_lo, **kw):
    """The restatement's run of the case, computed once."""
    key = (N, h, shared, cap_lo, tuple(sorted(kw.items())))
    if key not in _WANT:
        unary, _, _, pair_b, caps_b = _models(N, h, shared, cap_lo)
        _WANT[key] = BO.bp(unary, pair_b, caps_b, h, **kw)
    return _WANT[key]


def _solve(dev, N, h, shared, cap_lo, **kw):
    unary, pair, caps, _, _ = _models(N, h, shared, cap_lo)
    lab, det = _path(dev, N, h).solve_bp(torch.from_numpy(unary).to(dev), torch.from_numpy(np.ascontiguousarray(pair)).to(dev),
                                         torch.from_numpy(np.ascontiguousarray(caps)).to(dev), want_details=True, **kw)
    out = {k: v.cpu().numpy() for k, v in det.items()}
    out['labels'] = lab.cpu().numpy()
    assert out['labels'].dtype == np.int64 and out['beliefs'].dtype == np.float64
    assert out['status'].dtype == np.int32 and out['iters'].dtype == np.int32
    assert out['labels'].shape == out['beliefs'].shape == (B, N) and out['status'].shape == out['iters'].shape == (B,)
    return out


def _equal(got, want):
    assert np.array_equal(got['beliefs'], want['beliefs']), np.abs(got['beliefs'] - want['beliefs']).max()
    assert np.array_equal(got['labels'], want['labels'])
    assert np.array_equal(got['iters'], want['iters']) and np.array_equal(got['status'], want['status'])
    assert np.array_equal(got['labels'], (got['beliefs'] > 0).astype(np.int64))


@cases
@shapes
def test_undamped_run_is_the_restatement_bit_for_bit(dev, N, h, shared):
    """Caps 0..h (a cap of 0 sends -2^20, an integer: still exact).  Exact-zero beliefs (ties) decide 0 on both sides."""
    kw = dict(damping=0.0, max_iter=25, tol=0.0)
    got, want = _solve(dev, N, h, shared, 0, **kw), _want(N, h, shared, 0, **kw)
    assert (want['iters'] == 25).all() and (want['status'] == 3).all()
    _equal(got, want)


@cases
@shapes
def test_damped_run_is_the_restatement_bit_for_bit(dev, N, h, shared):
    """Damping 1/2 for 16 iterations: 24 fraction bits + 16 halvings + the integer bits stay under f64's 53.  Caps from 1: next to
    2^20 they would not."""
    kw = dict(damping=0.5, max_iter=16, tol=0.0)
    _equal(_solve(dev, N, h, shared, 1, **kw), _want(N, h, shared, 1, **kw))


@cases
@shapes
def test_general_damping_within_rounding(dev, N, h, shared):
    """Damping 0.3 is no dyadic value: products round, but in the order the restatement rounds them; only a library maximum or a
    compiler's choice could differ, and none is expected to (beliefs are O(10), one ulp 2e-15; next to a cap of 0 they reach 2^22,
    one ulp 9e-10).
    Labels are compared where the restatement's belief is not within 1e-7 of the tie; the seeds are such that the restatement alone
    keeps that exclusion within 1 % of the variables (checked below, on the restatement)."""
    kw = dict(damping=0.3, max_iter=25, tol=0.0)
    got, want = _solve(dev, N, h, shared, 0, **kw), _want(N, h, shared, 0, **kw)
    clear = np.abs(want['beliefs']) > 1e-7
    assert (~clear).mean() <= 0.01
    err = np.abs(got['beliefs'] - want['beliefs']).max()
    print('N=%d h=%d: max belief error %.3g, %d variables within 1e-7 of a tie' % (N, h, err, (~clear).sum()))
    assert err <= 1e-9
    assert np.array_equal(got['labels'][clear], want['labels'][clear])
    assert np.array_equal(got['iters'], want['iters']) and np.array_equal(got['status'], want['status'])


@cases
@shapes
def test_defaults_stop_where_the_restatement_stops(dev, N, h, shared):
    from fgnn_amd import _hip
    got, want = _solve(dev, N, h, shared, 0), _want(N, h, shared, 0)
    assert _hip.lib().fgnn_last_kernel().decode() == 'chain_budget_bp_kernel'
    same = (got['iters'] == want['iters']) & (got['status'] == want['status'])
    print('N=%d h=%d: iters and status equal on %d of %d; converged %d, iteration cap %d' %
          (N, h, same.sum(), B, (got['status'] == 0).sum(), (got['status'] == 3).sum()))
    assert same.mean() >= 0.99
    assert np.abs(got['beliefs'] - want['beliefs'])[same].max() <= 1e-9
    assert set(np.unique(got['status'])) <= {0, 3} and (got['iters'] <= 200).all()
    assert ((got['status'] == 3) <= (got['iters'] == 200)).all()


@pytest.mark.parametrize('family', ['pws', 'raw'])
def test_without_budgets_solve_bp_is_the_exact_map(dev, family):
    """Caps = h: a chain, a tree; N undamped parallel rounds carry every message from end to end."""
    N, h = 30, 9
    path = _path(dev, N, h)
    unary, pair, _ = path.lp_inputs(family, path.sample(256, family, seed=3, step=1))
    lab, det = path.solve_bp(unary, pair, h, max_iter=N, damping=0.0, tol=0.0, want_details=True)
    assert torch.equal(lab, path.solve_map(unary, pair, h))
    assert bool((det['iters'] == N).all()) and bool((det['status'] == 3).all())


def test_negative_cap_empty_batch_and_plain_return(dev):
    N, h = 12, 5
    rng = np.random.default_rng(3)
    unary, pair = _dyadic(rng, (4, N, 2), 0, 1), _dyadic(rng, (4, N - 1, 4), -1, 1)
    caps = np.full((4, N - h + 1), 2, np.int32)
    path = _path(dev, N, h)
    u, p = torch.from_numpy(unary).to(dev), torch.from_numpy(pair).to(dev)
    clean_lab, clean = path.solve_bp(u, p, torch.from_numpy(caps).to(dev), want_details=True)
    caps[2, 3] = -1
    lab, det = path.solve_bp(u, p, torch.from_numpy(caps).to(dev), want_details=True)
    assert int(det['status'][2]) == 2 and int(det['iters'][2]) == 0
    assert not bool(lab[2].any()) and not bool(det['beliefs'][2].any())
    keep = [0, 1, 3]
    assert torch.equal(lab[keep], clean_lab[keep])
    for k in ('beliefs', 'status', 'iters'):
        assert torch.equal(det[k][keep], clean[k][keep])
    assert bool((det['status'][keep] != 2).all())
    plain = path.solve_bp(u, p, 2)
    assert torch.is_tensor(plain) and torch.equal(plain, clean_lab)
    empty, d = path.solve_bp(torch.zeros(0, N, 2, device=dev), p[0], 2, want_details=True)
    assert empty.shape == (0, N) and empty.dtype == torch.int64
    assert d['beliefs'].shape == (0, N) and d['status'].shape == (0,) and d['iters'].shape == (0,)
    assert path.solve_bp(torch.zeros(0, N, 2, device=dev), p[0], 2).shape == (0, N)


@pytest.mark.parametrize('family', ['hops', 'pws', 'raw'])
def test_sample_with_bp_label(dev, family):
    N, h, n = 30, 9, 64
    path = _path(dev, N, h)
    plain = path.sample(n, family, seed=5, step=2, want_objective=True, lp_label=True)
    out = path.sample(n, family, seed=5, step=2, want_objective=True, lp_label=True, bp_label=True)
    assert len(out) == len(plain) + 1
    for a, b in zip(out[:-2], plain[:-1]):                                   # draws, the MAP label and the LP label unchanged
        assert torch.equal(a, b)
    assert torch.equal(out[-1], plain[-1])                                   # the objective stays last
    bp = out[-2]
    assert bp.shape == (n, N) and bp.dtype == torch.int64
    assert torch.equal(bp, path.solve_bp(*path.lp_inputs(family, plain)))
    only = path.sample(n, family, seed=5, step=2, bp_label=True)             # (..., MAP label, max-product label)
    assert len(only) == len(plain) - 1 and torch.equal(only[-1], bp) and torch.equal(only[-2], plain[-3])
    print('%s: max-product label = exact label on %.3f of the variables' % (family, (bp == plain[-3]).double().mean().item()))


def test_evaluate_with_the_bp_baseline(dev):
    from fgnn_amd.pgm_eval import build_model, evaluate, loop_figures, map_figures, score
    N, h, n = 30, 9, 64
    path = _path(dev, N, h)
    torch.manual_seed(0)
    model, edge = build_model('hops')
    model, edge = model.to(dev), tuple(m.to(dev) for m in edge)
    ts = path.sample(n, 'hops', seed=9, step=1 << 62, lp_label=True)
    base = evaluate(model, edge, ts, 'hops')
    r = evaluate(model, edge, ts, 'hops', bp=True)
    new = {'acc_bp', 'stddev_bp', 'pooled_acc_bp', 'bp', 'bp_converged'}
    assert set(r) == set(base) | new and not new & set(base)
    strip = lambda d: repr(sorted((k, v) for k, v in d.items() if k not in new))
    assert strip(r) == strip(base)
    label = ts[3]
    unary, pair, caps = path.lp_inputs('hops', ts)
    lab, det = path.solve_bp(unary, pair, caps, want_details=True)
    s = {k: v.cpu().numpy() for k, v in score(lab, label, unary, pair, caps, h).items()}
    smap = score(label, label, unary, pair, caps, h)['objective'].cpu().numpy()
    fig = loop_figures(s['correct'].astype(np.int64), None, s['correct'].astype(np.int64), N, 32)
    assert r['acc_bp'] == fig['acc_lp'] and r['stddev_bp'] == fig['stddev_lp'] and r['pooled_acc_bp'] == fig['pooled_acc_lp']
    assert repr(r['bp']) == repr(map_figures(s['correct'], s['feasible'], s['objective'], smap, N))
    assert r['bp_converged'] == float((det['status'] == 0).double().mean())
    assert r['pooled_acc_bp'] == float((lab == label).double().mean())
    short = evaluate(model, edge, ts, 'hops', eval_batch=24, bp=True, bp_args={'max_iter': 3})
    lab3, det3 = path.solve_bp(unary, pair, caps, max_iter=3, want_details=True)
    assert short['pooled_acc_bp'] == float((lab3 == label).double().mean())
    assert short['bp_converged'] == float((det3['status'] == 0).double().mean())
