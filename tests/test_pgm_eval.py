"""CPU: the synthetic-PGM evaluation's host side (csrc/pgm_eval.hip, fgnn_amd/pgm_eval.py):

  * the entry point validates its arguments before any launch (no device needed);
  * the numpy restatement the GPU tests hold the kernel to agrees with brute-force enumeration, and its test-loop arithmetic (and
    the module's) with the reference loop's statements run literally;
  * test sets in the reference's pickle stream parse in each family's item format;
  * the scripts' models and checkpoint dicts round-trip with strict loading;
  * the new kernel keeps everything in registers and LDS (compiler resource report, cross-compiled for gfx950)."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import pgm_eval_oracle as EO
import pgm_map_oracle as MO
import scratch_report as NS

EINVAL = -1                                    # FGNN_EINVAL


def test_score_entry_point_validates_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    one = ctypes.c_void_p(16)                  # non-NULL, never dereferenced on these paths

    def call(dec=one, kind=0, sb=60, cs=30, vs=1, label=one, lsb=30, unary=one, usb=60, pair=one, psb=0, caps=one, csb=0, B=4, N=30,
             h=9, correct=one, feasible=one, objective=one, nll=one, counts=one):
        return L.fgnn_chain_budget_score(dec, kind, sb, cs, vs, label, lsb, unary, usb, pair, psb, caps, csb, B, N, h, correct,
                                         feasible, objective, nll, counts, None)

    for kw in ('dec', 'label', 'unary', 'pair', 'caps'):
        assert call(**{kw: None}) == EINVAL, kw
    assert b'null pointer' in L.fgnn_last_error()
    assert call(kind=3) == _hip.EUNSUPPORTED and b'decision kind' in L.fgnn_last_error()
    assert call(kind=-1) == _hip.EUNSUPPORTED
    assert call(h=31) == _hip.EUNSUPPORTED and call(h=0) == _hip.EUNSUPPORTED and call(h=-2) == _hip.EUNSUPPORTED
    assert b'window' in L.fgnn_last_error()
    assert call(N=1025, h=9) == _hip.EUNSUPPORTED and b'1024' in L.fgnn_last_error()
    for kw in ('sb', 'cs', 'vs', 'lsb', 'usb', 'psb', 'csb'):
        assert call(**{kw: -1}) == EINVAL, kw
    assert b'negative stride' in L.fgnn_last_error()
    assert call(B=-1) == EINVAL and call(N=-1) == EINVAL
    assert call(kind=_hip.PGM_DEC_I64) == EINVAL and b'nll' in L.fgnn_last_error()        # nll needs logits
    # B = 0 is a no-op, whatever the pointers; every output is optional (the limits are accepted: the call fails at dec only)
    assert call(dec=None, label=None, unary=None, pair=None, caps=None, B=0) == 0
    assert call(dec=None, correct=None, feasible=None, objective=None, nll=None, counts=None, N=1024, h=1024) == EINVAL
    assert b'null pointer' in L.fgnn_last_error()


def test_python_score_refuses_bad_shapes_before_any_launch():
    from fgnn_amd.pgm_eval import score
    B, N = 3, 30
    u, p, lab = torch.zeros(B, N, 2), torch.zeros(N - 1, 4), torch.zeros(B, N, dtype=torch.int64)
    for dec, label, unary, what in ((torch.zeros(B, 2, N - 1, 1), lab, u, 'logits'), (torch.zeros(B, N, dtype=torch.int32), lab, u,
                                                                                       'decisions'),
                                    (torch.zeros(B, N - 1, dtype=torch.int64), lab, u, 'assignments'),
                                    (torch.zeros(B, 2, N, 1), lab.int(), u, 'int64'), (torch.zeros(B, 2, N, 1), lab, u[:2], 'samples'),
                                    (torch.zeros(B, 2, N, 1), lab, torch.zeros(B, N, 3), 'unary')):
        with pytest.raises(ValueError, match=what):
            score(dec, label, unary, p, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        score(torch.zeros(B, 2, N, 1), lab, u, p, 5)


def test_oracle_scores_agree_with_brute_force():
    """Feasibility and objective of every assignment of small chains (N <= 12) against enumeration, and the logits' decisions
    against torch.argmax (ties, +-0, NaN)."""
    rng = np.random.default_rng(0)
    for N, h in ((6, 2), (9, 3), (12, 4), (12, 12), (10, 5)):
        unary = rng.random((N, 2)).astype(np.float32)
        pair = rng.standard_normal((N - 1, 4)).astype(np.float32)
        caps = rng.integers(0, h + 1, N - h + 1)
        _, _, ok, sc = MO.brute_force(unary, pair, caps, h)
        X = (np.arange(1 << N)[:, None] >> np.arange(N)[None, :]) & 1
        K = len(X)
        label = X[rng.integers(0, K)][None].repeat(K, 0)
        correct, feas, obj, nll = EO.score(X, label, np.broadcast_to(unary, (K, N, 2)), np.broadcast_to(pair, (K, N - 1, 4)),
                                           np.broadcast_to(caps, (K, N - h + 1)), h, logits=False)
        assert nll is None
        assert np.array_equal(feas, ok)
        assert np.array_equal(correct, (X == label).sum(1))
        ref = unary[np.arange(N)[None, :], X].astype(np.float64).sum(1) + pair[np.arange(N - 1)[None, :], X[:, :-1] * 2 + X[:, 1:]].astype(np.float64).sum(1)
        assert np.allclose(obj, ref, rtol=1e-12, atol=0)
        assert np.allclose(np.where(ok, obj, -np.inf), sc, rtol=1e-12, atol=0)
    lg = rng.standard_normal((64, 2, 12)).astype(np.float32)
    lg[:8, 1] = lg[:8, 0]
    lg[8:12, 0], lg[8:12, 1] = 0.0, -0.0
    lg[12:16, 1] = np.nan
    lg[16:20, 0] = np.nan
    lg[20:24] = np.nan
    assert np.array_equal(EO.decisions(lg), torch.from_numpy(lg).argmax(1).numpy())
    lab = rng.integers(0, 2, (64, 12))
    t = torch.from_numpy(lg[24:]).permute(0, 2, 1).reshape(-1, 2)
    ce = torch.nn.functional.cross_entropy(t.double(), torch.from_numpy(lab[24:]).reshape(-1), reduction='none').reshape(40, 12).sum(1)
    assert np.allclose(EO.score(lg[24:], lab[24:], np.zeros((40, 12, 2)), np.zeros((40, 11, 4)), np.full((40, 10), 3), 3)[3],
                       ce.numpy(), rtol=1e-12)


def test_loop_arithmetic_agrees_with_the_reference_statements():
    """Per-batch mean and stdev from per-sample counts (oracle and fgnn_amd.pgm_eval.loop_figures) against the reference loop's
    statements run literally on the same arrays, 1000 samples in batches of 32 (a short last batch of 8)."""
    from fgnn_amd.pgm_eval import loop_figures
    rng = np.random.default_rng(1)
    n, N, bs = 1000, 30, 32
    logits = rng.standard_normal((n, 2, N, 1)).astype(np.float32)
    label = rng.integers(0, 2, (n, N))
    lp = np.where(rng.random((n, N)) < 0.9, label, 1 - label)
    correct, _, _, nll = EO.score(logits[..., 0], label, np.zeros((n, N, 2)), np.zeros((n, N - 1, 4)), np.full((n, N - 8), 9), 9)
    lp_correct = (lp == label).sum(1)
    batches = [(torch.from_numpy(logits[s:s + bs]), torch.from_numpy(label[s:s + bs]), torch.from_numpy(lp[s:s + bs]))
               for s in range(0, n, bs)]
    ref = EO.reference_loop(batches)
    mine = EO.loop_figures(correct, lp_correct, nll, N, bs)
    assert mine[:4] == ref[:4]                                       # the same float operations: bit for bit
    assert abs(mine[4] - ref[4]) <= 1e-6 * ref[4]                    # (the loss: f64 here, f32 in torch)
    f = loop_figures(correct, nll, lp_correct, N, bs)
    assert (f['acc'], f['acc_lp'], f['stddev'], f['stddev_lp']) == ref[:4]
    assert abs(f['loss'] - ref[4]) <= 1e-6 * ref[4] and f['batches'] == 32
    assert f['pooled_acc'] == correct.sum() / (n * N)
    g = loop_figures(correct[:20], None, None, N, bs)                 # one batch, no LP label: no stddev, LP unavailable (not 0)
    assert np.isnan(g['stddev']) and g['acc_lp'] is None and g['stddev_lp'] is None and g['loss'] is None


def _item(family, rng, N=30, h=9, lp=True):
    node = rng.random((2, N)).astype(np.float32)
    label = rng.integers(0, 2, N)
    a1 = rng.integers(0, 2, N) if lp else np.full(N, -1, np.int64)
    if family == 'raw':
        return node, label, a1
    pws = rng.random((4, N, 1)).astype(np.float32)
    if family == 'pws':
        return node, pws, label, a1
    hop = np.zeros((h, N, 1), np.float32)
    hop[rng.integers(0, h, N), np.arange(N), 0] = 1
    return node, pws, hop, label, a1


@pytest.mark.parametrize('family', ['raw', 'pws', 'hops'])
def test_load_test_set_parses_the_reference_item_formats(family, tmp_path):
    from fgnn_amd.pgm_eval import load_test_set
    rng = np.random.default_rng(2)
    for lp in (True, False):
        items = [_item(family, rng, lp=lp) for _ in range(7)]
        path = str(tmp_path / ('%s_%d.dat' % (family, lp)))
        with open(path, 'wb') as f:
            for it in items:
                pickle.dump(it, f)
        out = load_test_set(path, family, device='cpu')
        assert len(out) == {'raw': 3, 'pws': 4, 'hops': 5}[family]
        assert tuple(out[0].shape) == (7, 2, 30, 1) and out[0].dtype == torch.float32
        assert np.array_equal(out[0][..., 0].numpy(), np.stack([it[0] for it in items]))
        if family != 'raw':
            assert tuple(out[1].shape) == (7, 4, 30, 1) and np.array_equal(out[1].numpy(), np.stack([it[1] for it in items]))
        if family == 'hops':
            assert tuple(out[2].shape) == (7, 9, 30, 1) and np.array_equal(out[2].numpy(), np.stack([it[2] for it in items]))
        assert out[-2].dtype == torch.int64 and np.array_equal(out[-2].numpy(), np.stack([it[-2] for it in items]))
        if lp:
            assert np.array_equal(out[-1].numpy(), np.stack([it[-1] for it in items]))
        else:
            assert out[-1] is None                                       # all -1: no LP label, reported as unavailable
        assert len(load_test_set(path, family, size=3, device='cpu')[0]) == 3
        with pytest.raises(ValueError, match='holds 7 items'):
            load_test_set(path, family, size=8, device='cpu')
    with pytest.raises(ValueError, match='fields'):
        load_test_set(path, 'hops' if family != 'hops' else 'raw', device='cpu')


SCRIPT_FORMATS = [('raw', None), ('raw', 'mp_nn_comp'), ('raw', 'simple_gnn'), ('raw', 'iid'), ('pws', None), ('hops', None)]


@pytest.mark.parametrize('family,name', SCRIPT_FORMATS)
def test_checkpoints_in_the_script_formats_round_trip(family, name, tmp_path):
    from fgnn_amd.pgm_eval import EDGE_KEYS, build_model, load_checkpoint
    torch.manual_seed(0)
    model, edge = build_model(family, name)
    with torch.no_grad():
        for t in list(model.state_dict().values()) + [v for m in edge for v in m.state_dict().values()]:
            if t.is_floating_point():
                t.add_(torch.randn_like(t))
    ckpt = {'model_state_dict': model.state_dict(), 'optimizer_state_dict': {'state': {}, 'param_groups': []}, 'lr_sche': {},
            'epoch': 10, 'gcnt': 28130}
    for m, k in zip(edge, EDGE_KEYS[family]):
        ckpt[k] = m.state_dict()
    path = str(tmp_path / 'ckpt.pt')
    torch.save(ckpt, path)
    m2, e2 = load_checkpoint(path, family, name)
    for a, b in zip([model] + list(edge), [m2] + list(e2)):
        sa, sb = a.state_dict(), b.state_dict()
        assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    for k in EDGE_KEYS[family] + ('model_state_dict',):
        bad = dict(ckpt)
        del bad[k]
        torch.save(bad, path)
        with pytest.raises(KeyError, match=k):
            load_checkpoint(path, family, name)
    bad = dict(ckpt)
    bad['model_state_dict'] = {k: v for i, (k, v) in enumerate(ckpt['model_state_dict'].items()) if i}      # one tensor short
    torch.save(bad, path)
    with pytest.raises(RuntimeError, match='Missing key'):
        load_checkpoint(path, family, name)
    with pytest.raises(ValueError, match='model_name'):
        build_model(family, 'mp_nn_factor' if family == 'raw' else 'mp_nn')


@pytest.mark.skipif(not os.path.exists(NS.HIPCC), reason='no hipcc')
def test_score_kernel_has_no_scratch():
    rep = NS.scratch('pgm_eval.hip')
    hits = {k: v for k, v in rep.items() if 'chain_budget_score_kernel' in k}
    assert len(hits) == 3, rep                                       # f32, bf16 logits and int64 assignments
    assert not any(hits.values()), hits
