"""GPU: evaluating synthetic-PGM models on the device (csrc/pgm_eval.hip, fgnn_amd/pgm_eval.py):

  1. the scores equal the numpy restatement for f32 / bf16 logits through strided views and for int64 assignments, with each
     family's potentials shared and per sample, and across chunk boundaries of long chains;
  2. the MAP label scores feasible, all correct, with solve_map's objective; the LP label's accuracy is (lp == label).mean();
  3. scores do not depend on how a batch is cut or on the run; evaluate's logits do not depend on eval_batch beyond rounding;
  4. evaluate's figures equal the reference's test loop restated on the same model (batches of 32, file order);
  5. a written test set evaluates like the samples it came from;
  6. the command line runs end to end and prints JSON."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pgm_eval_oracle as EO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'factor-graph-neural-network_amd')
N, H = 30, 9


@pytest.fixture(scope='module')
def path(dev):
    from fgnn_amd import PgmDataPath
    return PgmDataPath(dev, N, H)


def _np(t):
    return t.detach().cpu().numpy()


def _dense(unary, pair, caps, B, N, h):
    """The potentials as [B, ...] numpy arrays (shared ones broadcast), for the oracle."""
    u = _np(unary).astype(np.float32)
    p = _np(torch.as_tensor(pair)).astype(np.float32).reshape(-1, N - 1, 4)
    c = np.asarray(_np(caps) if torch.is_tensor(caps) else np.full(N - h + 1, caps)).reshape(-1, N - h + 1)
    return u, np.broadcast_to(p, (B, N - 1, 4)), np.broadcast_to(c, (B, N - h + 1))


def _check(res, ref, counts, label_n):
    correct, feas, obj, nll = ref
    assert np.array_equal(_np(res['correct']), correct)
    assert np.array_equal(_np(res['feasible']), feas)
    assert np.allclose(_np(res['objective']), obj, rtol=1e-12, atol=0)
    if nll is not None:
        assert np.allclose(_np(res['nll']), nll, rtol=1e-6, atol=0, equal_nan=True)
    B = len(correct)
    assert _np(counts).tolist() == [B * label_n, int(correct.sum()), int(feas.sum()), int((correct == label_n).sum())]


def _logits(B, N, g, dev):
    """Random logits with ties, +-0 and NaNs, as two strided [B, 2, N, 1] views: every third variable of a wider tensor, and a
    [B, N, 2] tensor permuted (class stride 1)."""
    base = torch.randn(B, 2, N, 3, generator=g)
    base[:, 1, ::7, 1] = base[:, 0, ::7, 1]
    base[:5, 0, :, 1], base[:5, 1, :, 1] = 0.0, -0.0
    base[5, 1, ::4, 1] = float('nan')
    base[6, 0, ::5, 1] = float('nan')
    v1 = base.to(dev)[:, :, :, 1:2]
    v2 = torch.randn(B, N, 2, generator=g).to(dev).permute(0, 2, 1).unsqueeze(-1)
    return v1, v2


@pytest.mark.parametrize('family', ['raw', 'pws', 'hops'])
def test_scores_match_the_restatement(path, dev, family):
    from fgnn_amd.pgm_eval import score
    B = 333
    g = torch.Generator().manual_seed(3)
    out = path.sample(B, family, seed=11, step=5, lp_label=True)
    label, lp = out[-2], out[-1]
    unary, pair, caps = path.lp_inputs(family, out[:-1])
    variants = [(pair, caps)]
    if family == 'raw':               # shared pair and cap, and the same potentials per sample
        variants.append((pair.expand(B, N - 1, 4).contiguous(), torch.full((B, N - H + 1), 5, dtype=torch.int32, device=dev)))
    else:                             # per-sample pair; shared caps
        variants.append((pair, torch.randint(0, H + 1, (N - H + 1,), generator=g, dtype=torch.int32).to(dev)))
    rand_assign = torch.randint(0, 2, (B, N), generator=g).to(dev)
    for p, c in variants:
        u_np, p_np, c_np = _dense(unary, p, c, B, N, H)
        lab = _np(label)
        for v in _logits(B, N, g, dev):
            for dt in (torch.float32, torch.bfloat16):
                d = v.to(dt) if dt != torch.float32 else v
                cnt = torch.zeros(4, dtype=torch.int64, device=dev)
                res = score(d, label, unary, p, c, H, counts=cnt)
                _check(res, EO.score(_np(d[..., 0].float()), lab, u_np, p_np, c_np, H), cnt, N)
        for a in (rand_assign, lp, label):
            cnt = torch.zeros(4, dtype=torch.int64, device=dev)
            res = score(a, label, unary, p, c, H, counts=cnt)
            assert 'nll' not in res
            _check(res, EO.score(_np(a), lab, u_np, p_np, c_np, H, logits=False), cnt, N)


def test_long_chains_cross_chunk_boundaries(dev):
    """N = 200 (four 64-variable chunks), windows of 13 and of 70 (a window spanning two chunk edges), caps per sample."""
    from fgnn_amd import _hip
    g = torch.Generator().manual_seed(4)
    B, n = 97, 200
    for h in (13, 70):
        u = torch.rand(B, n, 2, generator=g)
        p = torch.randn(B, n - 1, 4, generator=g)
        c = torch.randint(0, h // 2 + 2, (B, n - h + 1), generator=g, dtype=torch.int32)
        lab = torch.randint(0, 2, (B, n), generator=g)
        lab[:10] = 0
        c[:10] = h                                                    # (those ten: feasible whatever the decisions)
        lg = torch.randn(B, 2, n, 1, generator=g) + 2.0 * (lab[:, None, :, None] * 2 - 1) * torch.tensor([-1., 1.])[None, :, None, None]
        d, labd, ud, pd, cd = (t.to(dev) for t in (lg, lab, u, p, c))
        outs = [torch.empty(B, dtype=dt, device=dev) for dt in (torch.int32, torch.uint8, torch.float64, torch.float64)]
        cnt = torch.zeros(4, dtype=torch.int64, device=dev)
        P = _hip._ptr
        _hip.check(_hip.lib().fgnn_chain_budget_score(P(d), _hip.PGM_DEC_F32, 2 * n, n, 1, P(labd), n, P(ud), 2 * n, P(pd), 4 * (n - 1),
                                                      P(cd), n - h + 1, B, n, h, *[P(o) for o in outs], P(cnt), _hip.stream_ptr()))
        ref = EO.score(lg[..., 0].numpy(), lab.numpy(), u.numpy(), p.numpy(), c.numpy(), h)
        assert 0 < ref[1].sum() < B                                   # both feasible and infeasible decisions
        _check(dict(zip(('correct', 'feasible', 'objective', 'nll'), outs)), ref, cnt, n)


def test_map_and_lp_labels(path, dev):
    from fgnn_amd.pgm_eval import score
    for family in ('raw', 'pws', 'hops'):
        out = path.sample(1000, family, seed=2, step=1, want_objective=True, lp_label=True)
        obj, lp, label = out[-1], out[-2], out[-3]
        unary, pair, caps = path.lp_inputs(family, out[:-2])
        cnt = torch.zeros(4, dtype=torch.int64, device=dev)
        r = score(label, label, unary, pair, caps, H, counts=cnt)
        assert bool(r['feasible'].all()) and bool((r['correct'] == N).all())
        assert torch.allclose(r['objective'], obj, rtol=1e-12, atol=0), float((r['objective'] - obj).abs().max())
        assert torch.equal(r['objective'], obj), 'the recursion order should give the MAP objective bit for bit'
        assert _np(cnt).tolist() == [1000 * N, 1000 * N, 1000, 1000]
        cnt.zero_()
        r = score(lp, label, unary, pair, caps, H, counts=cnt)
        assert int(cnt[1]) / int(cnt[0]) == float((lp == label).double().mean())
        assert bool((r['objective'][r['feasible']] <= obj[r['feasible']] * (1 + 1e-12)).all())        # nothing beats the MAP


def test_scores_do_not_depend_on_the_cut_or_the_run(path, dev):
    from fgnn_amd.pgm_eval import score
    B = 5000
    out = path.sample(B, 'hops', seed=7, step=0)
    label = out[-1]
    unary, pair, caps = path.lp_inputs('hops', out)
    logits = torch.randn(B, 2, N, 1, generator=torch.Generator().manual_seed(5)).to(dev)
    runs = []
    for chunk in (B, 1, 7, 4096, B):
        if chunk == 1:
            sub = 300                                                  # (one launch per sample: a prefix is enough)
        else:
            sub = B
        cnt = torch.zeros(4, dtype=torch.int64, device=dev)
        parts = {}
        for s in range(0, sub, chunk):
            e = min(sub, s + chunk)
            r = score(logits[s:e], label[s:e], unary[s:e], pair[s:e], caps[s:e], H, counts=cnt)
            for k, v in r.items():
                parts.setdefault(k, []).append(v)
        runs.append((sub, cnt.clone(), {k: torch.cat(v) for k, v in parts.items()}))
    full = runs[0][2]
    for sub, cnt, r in runs[1:]:
        for k in full:
            assert torch.equal(r[k], full[k][:sub]), k
        if sub == B:
            assert torch.equal(cnt, runs[0][1])
    ref = score(logits[:300], label[:300], unary[:300], pair[:300], caps[:300], H)
    assert torch.equal(ref['nll'], runs[1][2]['nll'])


def _same(a, b):
    """Equal figure dicts (NaN equal to NaN; logits left out)."""
    strip = lambda d: repr(sorted((k, v) for k, v in d.items() if k != 'logits'))
    return strip(a) == strip(b)


def _model(family, name=None, seed=0, dev=None):
    from fgnn_amd.pgm_eval import build_model
    torch.manual_seed(seed)
    model, edge = build_model(family, name)
    return model.to(dev), tuple(m.to(dev) for m in edge)


def test_eval_batch_changes_logits_only_by_rounding(path, dev):
    from fgnn_amd.pgm_eval import evaluate
    model, edge = _model('hops', dev=dev)
    ts = path.sample(2048, 'hops', seed=9, step=1 << 62, lp_label=True)
    a = evaluate(model, edge, ts, 'hops', 32, 32, return_logits=True)
    b = evaluate(model, edge, ts, 'hops', 32, 4096, return_logits=True)
    la, lb = a['logits'], b['logits']
    assert float((la - lb).abs().max()) <= 1e-5
    da, db = la.argmax(1), lb.argmax(1)
    near = (la[:, 1] - la[:, 0]).abs() < 1e-4
    assert bool(((da == db) | near).all())
    flips = int((da != db).sum())
    assert abs(a['pooled_acc'] - b['pooled_acc']) * 2048 * N <= flips
    if flips == 0:
        assert a['acc'] == b['acc'] and _same(a['model'], b['model'])
    assert a['acc_lp'] == b['acc_lp'] and _same(a['lp'], b['lp'])
    assert model.training and all(m.training for m in edge)          # training flags restored


def _reference_loop(model, edge, family, ts, bs=32):
    """The family script's test loop on the same model and items: batches of 32 in file order, tables by .repeat."""
    from fgnn_amd import tables
    *feats, label, lp = ts
    n = label.shape[0]
    dev = label.device
    t = lambda a: torch.from_numpy(a).to(dev)[None]
    batches = []
    for m in (model,) + tuple(edge):
        m.eval()
    with torch.no_grad():
        for s in range(0, n, bs):
            e = min(n, s + bs)
            nf = feats[0][s:e]
            b = nf.shape[0]
            if family == 'raw':
                idx, ef = tables.knn_table(N, 8)
                etype = edge[0](t(ef))
                pred = model(nf, t(idx).repeat(b, 1, 1), etype.repeat(b, 1, 1, 1))
            else:
                pw_idx, pw_ef = tables.pw_factor_table(N)
                if family == 'pws':
                    hi_idx, hi_ef, hf = tables.chain_high_table(N, 9)
                    high = torch.from_numpy(hf).to(dev)[None].repeat(b, 1, 1, 1)
                else:
                    hi_idx, hi_ef = tables.ring_hop_table(N, H)
                    high = feats[2][s:e]
                et_pw, et_hi = edge[0](t(pw_ef)), edge[1](t(hi_ef))
                pred, _ = model(nf, [feats[1][s:e], high], [[t(pw_idx).repeat(b, 1, 1), et_pw.repeat(b, 1, 1, 1)],
                                                             [t(hi_idx).repeat(b, 1, 1), et_hi.repeat(b, 1, 1, 1)]])
            batches.append((pred.cpu(), label[s:e].cpu(), lp[s:e].cpu()))
    for m in (model,) + tuple(edge):
        m.train()
    return EO.reference_loop(batches)


@pytest.mark.parametrize('family,name', [('hops', None), ('pws', None), ('raw', 'simple_gnn')])
def test_evaluate_matches_the_reference_loop(path, dev, family, name):
    from fgnn_amd.pgm_eval import evaluate
    model, edge = _model(family, name, seed=1, dev=dev)
    ts = path.sample(2048, family, seed=21, step=1 << 62, lp_label=True)
    r = evaluate(model, edge, ts, family, batch_size=32, eval_batch=32)
    ref = _reference_loop(model, edge, family, ts)
    got = (r['acc'], r['acc_lp'], r['stddev'], r['stddev_lp'], r['loss'])
    print('%s %s: acc %.6f acc_lp %.6f stddev %.6f stddev_lp %.6f loss %.6f | model feasible %.4f gap %.4f | lp feasible %.4f gap %.4f'
          % ((family, name) + got + (r['model']['feasible'], r['model']['mean_gap'], r['lp']['feasible'], r['lp']['mean_gap'])))
    for a, b, what in zip(got, ref, ('acc', 'acc_lp', 'stddev', 'stddev_lp', 'loss')):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (what, a, b)
    assert r['map_feasible'] == 1.0 and r['batches'] == 64
    for who in ('model', 'lp'):
        f = r[who]
        assert 0 <= f['exact_map'] <= f['optimal'] <= f['feasible'] <= 1
        assert np.isnan(f['mean_gap']) or f['mean_gap'] >= -1e-12


def test_written_test_set_evaluates_like_its_samples(dev, tmp_path):
    from fgnn_amd import PgmDataPath
    from fgnn_amd.pgm_eval import TEST_STEP, evaluate, load_test_set, make_test_set
    for family in ('hops', 'raw'):
        model, edge = _model(family, 'simple_gnn' if family == 'raw' else None, seed=2, dev=dev)
        p = str(tmp_path / ('%s.dat' % family))
        make_test_set(p, family, 300, seed=3, device=dev)
        ts = load_test_set(p, family, device=dev)
        mem = PgmDataPath(dev, N, H).sample(300, family, seed=3, step=TEST_STEP, lp_label=True)
        assert len(ts) == len(mem) and all(torch.equal(a, b) for a, b in zip(ts, mem))
        a = evaluate(model, edge, ts, family, eval_batch=128)
        b = evaluate(model, edge, mem, family, eval_batch=128)
        c = evaluate(model, edge, p, family, eval_batch=128)
        assert _same(a, b) and _same(a, c)


def test_command_line_end_to_end(dev, tmp_path):
    from fgnn_amd.pgm_eval import EDGE_KEYS, evaluate, load_test_set
    model, edge = _model('hops', seed=4, dev=dev)
    ck = str(tmp_path / 'ckpt.pt')
    d = {'model_state_dict': model.state_dict(), 'optimizer_state_dict': {}, 'lr_sche': {}, 'epoch': 1, 'gcnt': 0}
    d.update({k: m.state_dict() for k, m in zip(EDGE_KEYS['hops'], edge)})
    torch.save(d, ck)
    ts = str(tmp_path / 'hop_test.dat')
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get('PYTHONPATH', ''))
    run = lambda args: subprocess.run([sys.executable, '-m', 'fgnn_amd.pgm_eval'] + args, capture_output=True, text=True,
                                      timeout=300, env=env, cwd=str(tmp_path))
    p = run(['--family', 'hops', '--make_test_set', ts, '--num', '512', '--seed', '1'])
    assert p.returncode == 0, p.stderr[-2000:]
    p = run(['--family', 'hops', '--test_path', ts, '--model_path', ck, '--json'])
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r['n'] == 512 and r['batches'] == 16 and 0 <= r['acc'] <= 1 and 0 <= r['model']['feasible'] <= 1
    mine = evaluate(model, edge, load_test_set(ts, 'hops', device=dev), 'hops')
    assert abs(r['acc'] - mine['acc']) <= 1e-12 and abs(r['acc_lp'] - mine['acc_lp']) <= 1e-12
    p = run(['--family', 'hops', '--test_path', ts, '--model_path', ck, '--test_size', '100'])
    assert p.returncode == 0 and 'testing result: acc = ' in p.stdout and 'feasible' in p.stdout, p.stdout + p.stderr[-2000:]
