"""GPU: the LDPC trainer (fgnn_amd/ldpc_train.py) and the two entry points under it (include/fgnn_hip_ldpc_train.h) — the one-launch
sampler against its numpy restatement (tests/ldpc_train_oracle.py) and against the kernels it is made of, the loss parts against
``decoding_loss`` and torch, and the loop: graph against eager, the loop against its parts, learning, resume, checkpoints, the
capture fallback and the command line."""
import contextlib
import functools
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import ldpc_train_oracle as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'factor-graph-neural-network_amd')
BIG = (0x1234567887654321, 2 ** 33 + 5)


@pytest.fixture(scope='module')
def path(dev):
    from fgnn_amd.datapath import LdpcDataPath
    return LdpcDataPath(dev)


@functools.lru_cache(maxsize=None)
def _restated(B, seed, step, snr):
    """The restatement of one batch, computed once per (B, seed, step, fixed SNR or None) and shared (read-only)."""
    G = H.load('ldpc_datapath.npz')['G']
    out = R.sample_batch(G, B, seed, step, snr_choices=R.SNR_CHOICES if snr is None else (snr,))
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. the sampler -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('snr', [None, 2], ids=['snr_drawn', 'snr_2'])
@pytest.mark.parametrize('seed, step', [(0, 0), BIG], ids=['seed0_step0', 'seed64_step2p33'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('B', [1, 3, 65, 300])
def test_sampler_equals_its_restatement_and_the_kernels_it_is_made_of(B, dtype, seed, step, snr, path):
    from fgnn_amd import _hip
    d = path.sample_rng(B, seed=seed, step=step, dtype=dtype, snr_db=snr)
    assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_features_kernel<rng, draw>'
    cw_ref, snr_ref, sb_ref, y_ref = _restated(B, seed, step, snr)
    # the draws: exact
    assert d.cw.dtype == torch.uint8 and np.array_equal(d.cw.cpu().numpy(), cw_ref)
    assert d.snr_db.dtype == torch.float32 and np.array_equal(d.snr_db.cpu().numpy(), snr_ref)
    assert d.sigma_b.dtype == torch.float32 and np.array_equal(d.sigma_b.cpu().numpy(), sb_ref)
    if snr is not None:
        assert set(snr_ref.tolist()) == {2.0}
    # the codeword is the encoder's; the label is its message part, as the loss reads it
    assert torch.equal(d.cw, path.encode(d.cw[:, :48]))
    assert d.label.dtype == torch.float32 and d.label.shape == (B, 48) and torch.equal(d.label, d.cw[:, :48].float())
    # the channel and the gather are the rng feature kernel's: the same bits for the drawn codewords and classes
    y, node, hop, e1, e2 = path.channel_features(d.cw, d.snr_db, d.sigma_b, 0.05, dtype=dtype, kernel_rng=(seed, step))
    for name, got, want in (('y', d.y, y), ('node', d.node_feature, node), ('hop', d.hop_feature, hop), ('ef_f2v', d.efeature_f2v, e1),
                            ('ef_v2f', d.efeature_v2f, e2)):
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), name
    assert d.node_feature.dtype == dtype and d.y.dtype == torch.float32
    # ... and the restated channel on the restated draws, to f32 rounding of the transcendental functions
    err = np.abs(d.y.cpu().numpy() - y_ref).max()
    assert err <= 2e-5 * np.abs(y_ref).max(), err
    # the reference's item order, the index tables shared by the batch
    assert d._fields[:8] == ('node_feature', 'hop_feature', 'nn_idx_f2v', 'nn_idx_v2f', 'efeature_f2v', 'efeature_v2f', 'label', 'sigma_b')
    assert d._fields[8:10] == ('snr_db', 'cw')
    assert d.nn_idx_f2v.shape == (B, 96, 3) and d.nn_idx_v2f.shape == (B, 48, 6) and d.nn_idx_f2v.dtype == torch.int64
    assert (d.nn_idx_f2v.stride(0) == 0 and d.nn_idx_v2f.stride(0) == 0) or B == 1
    assert d.nn_idx_f2v.data_ptr() == path.nn_idx_f2v.data_ptr() and d.sigma_b.shape == (B,)


@pytest.mark.parametrize('seed, step', [(0, 0), (7, 3)])
def test_sampler_draws_equal_the_restatement_at_60000_codewords(seed, step, path):
    """The batches whose statistics the CPU suite checks on the restatement (tests/test_ldpc_train.py): the kernel draws exactly those
    messages and classes, so the statistics are the kernel's."""
    d = path.sample_rng(60000, seed=seed, step=step, dtype=torch.bfloat16)
    s, i_snr, i_sigma = R.sample_draws(60000, seed, step)
    assert np.array_equal(d.cw[:, :48].cpu().numpy(), s) and np.array_equal(d.label.cpu().numpy(), s.astype(np.float32))
    assert np.array_equal(d.snr_db.cpu().numpy(), np.asarray(R.SNR_CHOICES, np.float32)[i_snr])
    assert np.array_equal(d.sigma_b.cpu().numpy(), np.asarray(R.SIGMA_CHOICES, np.float32)[i_sigma])
    assert torch.equal(d.cw, path.encode(d.cw[:, :48]))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_sampler_is_cut_invariant_and_draws_anew_every_step(dtype, path):
    seed, step = BIG
    a = path.sample_rng(65, seed=seed, step=step, dtype=dtype)
    b = path.sample_rng(16, seed=seed, step=step, dtype=dtype)
    for name, x, y in zip(a._fields, a, b):
        assert torch.equal(x[:16], y), name
    c = path.sample_rng(65, seed=seed, step=step + 1, dtype=dtype)
    same = float((a.label == c.label).float().mean())
    print('equal message bits between step and step + 1: %.4f' % same)
    assert not torch.equal(a.label, c.label) and 0.4 <= same <= 0.6
    assert not torch.equal(a.y, c.y)
    other = path.sample_rng(65, seed=seed + 1, step=step, dtype=dtype)
    assert not torch.equal(a.label, other.label)
    assert path.sample_rng(0, dtype=dtype).label.shape == (0, 48)


def test_sampler_writes_into_a_previous_result(path):
    from fgnn_amd import _hip
    first = path.sample_rng(65, seed=3, step=0, dtype=torch.bfloat16)
    ptrs = [t.data_ptr() for t in first]
    was = [t.clone() for t in first]
    _hip.call('fgnn_ldpc_encode', first.cw[:, :48].contiguous(), path.gmask, 65, 48, 48, torch.empty_like(first.cw))
    again = path.sample_rng(65, seed=3, step=1, dtype=torch.bfloat16, out=first)
    assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_features_kernel<rng, draw>'      # ONE launch, and it is the sampler's
    assert again is first and [t.data_ptr() for t in again] == ptrs
    fresh = path.sample_rng(65, seed=3, step=1, dtype=torch.bfloat16)
    for name, x, y, old in zip(first._fields, first, fresh, was):
        assert torch.equal(x, y), name
        if name not in ('nn_idx_f2v', 'nn_idx_v2f'):
            assert not torch.equal(x, old), name
    with pytest.raises(ValueError):
        path.sample_rng(64, seed=3, step=1, dtype=torch.bfloat16, out=first)
    with pytest.raises(ValueError):
        path.sample_rng(65, seed=3, step=1, dtype=torch.float32, out=first)


# ---- 2. the loss parts --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('B', [1, 7, 300])
def test_loss_parts_against_decoding_loss_and_torch(B, dtype, dev):
    """B = 300: 14400 logits, more than one workgroup of partials."""
    from fgnn_amd.ldpc import decoding_loss, decoding_loss_parts
    g = torch.Generator().manual_seed(B)
    logits = torch.randn(B, 48, generator=g) * 4
    flat = logits.view(-1)
    flat[0::14] = 0.0                               # every 7th logit a zero: +0.0 and -0.0 alternately (both decide 0)
    flat[7::14] = -0.0
    logits = logits.to(dtype).to(dev)
    pred = torch.rand(B, 1, generator=g).mul(3).to(dev)
    label = torch.randint(0, 2, (B, 48), generator=g).float().to(dev)
    sigma_b = torch.randint(0, 6, (B,), generator=g).float().to(dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    l1, p1 = logits.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    loss, parts = decoding_loss_parts(l1, p1, label, sigma_b, 0.1, counts)
    l2, p2 = logits.clone().requires_grad_(True), pred.clone().requires_grad_(True)
    plain = decoding_loss(l2, p2, label, sigma_b, 0.1)
    assert loss.shape == () and parts.shape == (3,) and parts.dtype == torch.float32 and not parts.requires_grad and loss.requires_grad
    assert torch.equal(parts[0], plain.detach()) and torch.equal(loss.detach(), plain.detach())
    x64 = logits.double().view(-1)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x64, label.double().view(-1))
    mse = torch.nn.functional.mse_loss(pred.double().view(-1), torch.pow(10.0, sigma_b.double() / 20))
    print('B', B, 'parts', parts.tolist(), 'f64 bce', float(bce), 'mse', float(mse))
    assert abs(float(parts[1]) - float(bce)) <= 1e-5 * max(1.0, abs(float(bce)))
    assert abs(float(parts[2]) - float(mse)) <= 1e-5 * max(1.0, abs(float(mse)))
    right = int(((logits.float() > 0) == label.bool()).sum())
    assert counts.tolist() == [B * 48, right]
    assert int((logits.float() == 0).sum()) >= B * 48 // 7
    loss2, parts2 = decoding_loss_parts(logits, pred, label, sigma_b, 0.1, counts)      # counts are added to
    assert counts.tolist() == [2 * B * 48, 2 * right] and torch.equal(parts2, parts)
    assert torch.equal(decoding_loss_parts(logits, pred, label, sigma_b, 0.1)[1], parts)  # ... and optional
    (loss * 1.5).backward()
    (plain * 1.5).backward()
    assert torch.equal(l1.grad, l2.grad) and torch.equal(p1.grad, p2.grad) and l1.grad.dtype == dtype


# ---- 3. the loop --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def test_set(path):
    return path.make_test_set(4, baseline=False)


@pytest.fixture(scope='module')
def runs(dev, test_set, tmp_path_factory):
    """One eager and one graphed run of the same settings, shared: 2 epochs x 6 steps, batch 384, bf16."""
    from fgnn_amd import ldpc_train
    out = {}
    for name, graph in (('eager', False), ('graphed', True)):
        d = str(tmp_path_factory.mktemp(name))
        with contextlib.redirect_stdout(io.StringIO()) as log:
            out[name] = ldpc_train.train(n_epochs=2, batch_size=384, steps_per_epoch=6, dtype=torch.bfloat16, seed=0, out_dir=d, graph=graph,
                                         log_every=4, test_set=test_set, device=dev)
        out[name]['log'] = log.getvalue()
    return out


@pytest.mark.parametrize('which', ['eager', 'graphed'])
def test_loop_counts_its_steps_and_reports_the_last_window(which, runs):
    r = runs[which]
    assert r['steps'] == r['gcnt'] == 12 and len(r['losses']) == 12 and all(np.isfinite(r['losses']))
    assert r['graphed'] == (which == 'graphed') and r['seconds'] > 0
    assert 0.0 <= r['acc'] <= 1.0 and np.isfinite(r['loss']) and np.isfinite(r['sigma_b_loss'])
    # log_every = 4 with 6 steps per epoch: a line whenever gcnt reaches 4, 8, 12 (train_ldpc.py:242 counts over the run, not per
    # epoch), so the last window is the last four steps; total = BCE + 0.1 MSE per step, so the window's BCE mean + 0.1 x its MSE
    # mean is the mean of its totals (f32 values: 1e-5 relative).  (The BCE mean itself: test_loop_equals_its_parts.)
    want = float(np.mean(r['losses'][-4:]))
    got = r['loss'] + 0.1 * r['sigma_b_loss']
    print(which, 'losses', r['losses'], 'loss', r['loss'], 'sigma_b_loss', r['sigma_b_loss'], 'acc', r['acc'])
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want))
    assert 0.0 < r['loss'] < want
    lines = [l for l in r['log'].splitlines() if l.startswith('epoch = ')]
    assert [l.split(' loss = ')[0] for l in lines] == ['epoch = 0 bcnt = 3', 'epoch = 1 bcnt = 1', 'epoch = 1 bcnt = 5']
    assert all(' acc = ' in l and ' sigma_b_loss = ' in l for l in lines)
    assert lines[-1] == 'epoch = 1 bcnt = 5 loss = {} acc = {} sigma_b_loss = {}'.format(r['loss'], r['acc'], r['sigma_b_loss'])
    assert os.path.basename(r['checkpoint']) == 'FactorNN_nn_factor_epoches_2_snr_None.pt' and os.path.exists(r['checkpoint'])


def test_graphed_loop_starts_like_the_eager_one(runs):
    assert runs['graphed']['graphed'] and not runs['eager']['graphed']
    assert runs['graphed']['losses'][:3] == runs['eager']['losses'][:3]


def test_log_lines_come_every_log_every_steps_across_epochs(dev, tmp_path):
    """Fewer steps per epoch than ``log_every`` (the quick start's 3 steps at batch 4096): 4 epochs x 3 steps with log_every = 5 print at
    gcnt = 5 and 10, i.e. in epochs 1 and 3; each line averages the five steps before it, and the two steps behind the last line are
    the result's last window.  A resumed run keeps the count: from gcnt = 6 the next line is at gcnt = 10 (over the steps since the resume)."""
    from fgnn_amd import ldpc_train
    kw = dict(batch_size=96, steps_per_epoch=3, dtype=torch.float32, seed=4, log_every=5, graph=False, device=dev)
    with contextlib.redirect_stdout(io.StringIO()) as log:
        r = ldpc_train.train(n_epochs=4, out_dir=str(tmp_path / 'whole'), **kw)
    lines = [l for l in log.getvalue().splitlines() if l.startswith('epoch = ')]
    assert [l.split(' loss = ')[0] for l in lines] == ['epoch = 1 bcnt = 1', 'epoch = 3 bcnt = 0']
    assert r['steps'] == r['gcnt'] == 12 and len(r['losses']) == 12
    field = lambda l, name: float(l.split(' %s = ' % name)[1].split(' ')[0])
    for l, win in zip(lines, (r['losses'][0:5], r['losses'][5:10])):
        want = float(np.mean(win))
        assert abs(field(l, 'loss') + 0.1 * field(l, 'sigma_b_loss') - want) <= 1e-5 * max(1.0, abs(want)), l
        assert 0.0 <= field(l, 'acc') <= 1.0
    want = float(np.mean(r['losses'][10:]))
    assert abs(r['loss'] + 0.1 * r['sigma_b_loss'] - want) <= 1e-5 * max(1.0, abs(want))
    with contextlib.redirect_stdout(io.StringIO()) as log:
        two = ldpc_train.train(n_epochs=2, out_dir=str(tmp_path / 'parts'), **kw)
        rest = ldpc_train.train(n_epochs=4, out_dir=str(tmp_path / 'parts'), model_path=two['checkpoint'], **kw)
    again = [l for l in log.getvalue().splitlines() if l.startswith('epoch = ')]
    # the line at gcnt = 5 is the same; the resumed run's window starts where it resumed: its line at gcnt = 10 averages steps 6 .. 9
    assert again[0] == lines[0] and [l.split(' loss = ')[0] for l in again] == ['epoch = 1 bcnt = 1', 'epoch = 3 bcnt = 0']
    assert two['losses'] + rest['losses'] == r['losses']
    want = float(np.mean(r['losses'][6:10]))
    assert abs(field(again[1], 'loss') + 0.1 * field(again[1], 'sigma_b_loss') - want) <= 1e-5 * max(1.0, abs(want))
    assert (rest['loss'], rest['sigma_b_loss'], rest['acc']) == (r['loss'], r['sigma_b_loss'], r['acc'])
    # no log lines asked for: none printed, the result is the same
    with contextlib.redirect_stdout(io.StringIO()) as log:
        quiet = ldpc_train.train(n_epochs=4, out_dir=str(tmp_path / 'quiet'), **dict(kw, log_every=0))
    assert 'epoch = ' not in log.getvalue() and quiet['losses'] == r['losses']


def test_checkpoint_loads_evaluates_and_counts_adams_steps(runs, test_set, dev):
    from fgnn_amd import ldpc_eval, ldpc_train
    r = runs['eager']
    ck = torch.load(r['checkpoint'], map_location='cpu', weights_only=True)
    assert set(ck) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt'} and ck['epoch'] == 2 and ck['gcnt'] == 12
    model = ldpc_train.build_model('max')
    model.load_state_dict(ck['model_state_dict'], strict=True)
    res = ldpc_eval.evaluate(model.to(dev), test_set, dtype=torch.bfloat16)
    assert 0.0 <= res['ber'] <= 1.0 and res['counts'][-1][0] == 120 * 48
    assert r['ber'] == res['ber'] and np.array_equal(r['err_class'], res['err_class'], equal_nan=True)
    assert str(res['ber']) in r['log']
    state = ck['optimizer_state_dict']['state']
    assert state and all(int(st['step']) == 12 for st in state.values())
    assert ck['lr_sche']['last_epoch'] == 2


def test_loop_equals_its_parts(dev, tmp_path):
    """Four eager f32 steps of ``train`` against the same four written out: sample_rng, LDPCModel, decoding_loss, FastAdam at epoch
    0's rate.  The losses are the same bits."""
    from fgnn_amd import ldpc_train
    from fgnn_amd.datapath import LdpcDataPath
    from fgnn_amd.fastpath import FastAdam
    from fgnn_amd.graph import state_moved
    from fgnn_amd.ldpc import decoding_loss
    with contextlib.redirect_stdout(io.StringIO()):
        r = ldpc_train.train(n_epochs=1, batch_size=96, steps_per_epoch=4, dtype=torch.float32, seed=5, out_dir=str(tmp_path), graph=False,
                             device=dev)
    torch.manual_seed(5)
    model = ldpc_train.build_model('max').to(dev).train()
    opt = FastAdam(model.parameters(), lr=1e-2 * ldpc_train.lr_sched(0), weight_decay=1e-8)
    state_moved()
    path = LdpcDataPath(dev)
    losses, bce, mse, right = [], [], [], 0
    for step in range(4):
        b = path.sample_rng(96, seed=5, step=step, dtype=torch.float32)
        opt.zero_grad()
        logits, pred = model(*b[:6])
        loss = decoding_loss(logits, pred, b.label, b.sigma_b, 0.1)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        # what the script logs per step (train_ldpc.py:222-225,235-237), from the same logits, in f64
        x = logits.detach().double()
        bce.append(float(torch.nn.functional.binary_cross_entropy_with_logits(x.view(-1), b.label.double().view(-1))))
        mse.append(float(torch.nn.functional.mse_loss(pred.detach().double().view(-1), torch.pow(10.0, b.sigma_b.double() / 20))))
        right += int(((logits.detach() > 0).long() == b.label.long()).sum())
    print('train', r['losses'], 'written out', losses)
    assert not r['graphed'] and r['losses'] == losses and len(set(losses)) == 4
    # four steps, log_every = 10: the one window is the whole run.  `loss` is its mean BCE, `sigma_b_loss` its mean MSE (1e-5, the
    # tolerance of the parts against f64 torch), `acc` the exact share of bits decided as the label says
    print('loss', r['loss'], 'mean BCE', np.mean(bce), 'sigma_b_loss', r['sigma_b_loss'], 'mean MSE', np.mean(mse), 'acc', r['acc'])
    assert abs(r['loss'] - np.mean(bce)) <= 1e-5 * max(1.0, np.mean(bce))
    assert abs(r['sigma_b_loss'] - np.mean(mse)) <= 1e-5 * max(1.0, np.mean(mse))
    assert abs(np.mean(bce) - np.mean(mse)) > 1e-3                 # (a swap of the two columns would show)
    assert r['acc'] == right / (4 * 96 * 48)


def test_loop_learns(dev, tmp_path):
    """60 graphed steps at batch 1024 with lr = 1e-1: epoch 0 runs at 1e-3, the rate tests/test_convergence_gpu.py trains this model at."""
    from fgnn_amd import ldpc_train
    with contextlib.redirect_stdout(io.StringIO()):
        r = ldpc_train.train(n_epochs=1, batch_size=1024, steps_per_epoch=60, dtype=torch.bfloat16, seed=0, out_dir=str(tmp_path), lr=1e-1,
                             device=dev)
    first, last = float(np.mean(r['losses'][:10])), float(np.mean(r['losses'][-10:]))
    print('mean loss of the first 10 steps %.5f, of the last 10 %.5f (graphed: %s)' % (first, last, r['graphed']))
    assert r['graphed'] and r['steps'] == 60
    assert last < first


def test_resumed_run_equals_the_run_in_one_go(dev, tmp_path):
    from fgnn_amd import ldpc_train
    kw = dict(batch_size=96, steps_per_epoch=4, seed=2, graph=False, device=dev)
    with contextlib.redirect_stdout(io.StringIO()):
        whole = ldpc_train.train(n_epochs=2, out_dir=str(tmp_path / 'whole'), **kw)
        one = ldpc_train.train(n_epochs=1, out_dir=str(tmp_path / 'parts'), **kw)
        two = ldpc_train.train(n_epochs=2, out_dir=str(tmp_path / 'parts'), model_path=one['checkpoint'], **kw)
    assert one['checkpoint'].endswith('epoches_1_snr_None.pt') and two['checkpoint'].endswith('epoches_2_snr_None.pt')
    assert (one['steps'], one['gcnt'], two['steps'], two['gcnt']) == (4, 4, 4, 8) and whole['gcnt'] == 8
    assert one['losses'] + two['losses'] == whole['losses']
    a, b = (torch.load(r['checkpoint'], map_location='cpu', weights_only=True) for r in (two, whole))
    assert a['epoch'] == b['epoch'] == 2 and a['gcnt'] == b['gcnt'] == 8
    assert a['model_state_dict'].keys() == b['model_state_dict'].keys()
    for k in a['model_state_dict']:
        assert torch.equal(a['model_state_dict'][k], b['model_state_dict'][k]), k
    sa, sb = a['optimizer_state_dict']['state'], b['optimizer_state_dict']['state']
    assert sa.keys() == sb.keys() and len(sa) > 100
    for k in sa:
        assert torch.equal(sa[k]['exp_avg_sq'], sb[k]['exp_avg_sq']) and torch.equal(sa[k]['exp_avg'], sb[k]['exp_avg']), k
    assert a['lr_sche']['last_epoch'] == 2
    assert a['optimizer_state_dict']['param_groups'][0]['lr'] == 1e-2 * ldpc_train.lr_sched(2)


def test_a_failed_capture_falls_back_to_what_graph_false_gives(dev, tmp_path, monkeypatch):
    """graph=True with a capture that raises after one warm-up run of the step: one line on stderr, then eager steps from the
    BatchNorm buffers and counts of graph=False — the same losses, window accuracy and final checkpoint, bit for bit."""
    from fgnn_amd import graph, ldpc_train
    kw = dict(n_epochs=1, batch_size=96, steps_per_epoch=3, dtype=torch.bfloat16, seed=1, device=dev)
    with contextlib.redirect_stdout(io.StringIO()):
        want = ldpc_train.train(graph=False, out_dir=str(tmp_path / 'eager'), **kw)
    real, runs = graph.StepGraph, []

    def once_then_raise(fn, **kwargs):
        def step():
            if runs:
                raise RuntimeError('no capture today')
            runs.append(fn())
        return real(step, **kwargs)
    monkeypatch.setattr(graph, 'StepGraph', once_then_raise)
    err = io.StringIO()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(err):
        got = ldpc_train.train(graph=True, out_dir=str(tmp_path / 'fallback'), **kw)
    said = [l for l in err.getvalue().splitlines() if 'capture failed' in l]
    assert len(said) == 1 and 'no capture today' in said[0] and 'running eagerly' in said[0]
    assert len(runs) == 1 and not got['graphed'] and not want['graphed']
    assert len(want['losses']) == 3 and got['losses'] == want['losses']
    assert (got['acc'], got['loss'], got['sigma_b_loss']) == (want['acc'], want['loss'], want['sigma_b_loss'])
    a, b = (torch.load(r['checkpoint'], map_location='cpu', weights_only=True)['model_state_dict'] for r in (got, want))
    assert a.keys() == b.keys() and any('num_batches_tracked' in k or 'running' in k for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_command_line_trains_and_writes_the_checkpoint(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, '-m', 'fgnn_amd.ldpc_train', '--n_epochs', '1', '--batch_size', '96', '--steps_per_epoch', '2',
                        '--json', '--out_dir', str(tmp_path)], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['steps'] == 2 and res['gcnt'] == 2 and 'losses' not in res
    assert res['checkpoint'] == os.path.join(str(tmp_path), 'FactorNN_nn_factor_epoches_1_snr_None.pt') and os.path.exists(res['checkpoint'])
    assert all(l.startswith(('epoch = ', '{')) for l in r.stdout.strip().splitlines())          # stdout: log lines and the result only
