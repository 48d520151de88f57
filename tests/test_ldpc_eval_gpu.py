"""GPU: evaluating LDPC decoders on the device (csrc/ldpc_eval.hip, fgnn_ldpc_received_features, fgnn_amd/ldpc_eval.py):

  1. features from a stored received word equal those the channel call made from the same word, and the host restatement's;
  2. the error counts equal the numpy restatement of train_ldpc.py:289-327, integer for integer, and accumulate deterministically;
  3. test sets follow data_generate/ldpc.py (order, codewords, channel statistics, sum-product table) and are reproducible;
  4. a written test set evaluates like the dict it came from;
  5. evaluate() counts what the reference's loop (host features, batches of 100) counts on the same model;
  6. the command line prints what evaluate() returns."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import ldpc_eval_oracle as EO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'factor-graph-neural-network_amd')


@pytest.fixture(scope='module')
def path(dev):
    from fgnn_amd.datapath import LdpcDataPath
    return LdpcDataPath(dev)


@pytest.fixture(scope='module')
def model(dev):
    import fgnn_amd
    with contextlib.redirect_stdout(io.StringIO()):
        m = fgnn_amd.LDPCModel(2, 6, 4, aggregator='max')
    m.load_state_dict(H.fill_state_dict(m.state_dict(), gain=2.0))
    return m.to(dev).eval()


@pytest.fixture(scope='module')
def small_set(path):
    return path.make_test_set(4, seed=11, baseline=False)


# ---- 1. features -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [1, 333, 4096])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('rng', [False, True], ids=['noise', 'kernel_rng'])
def test_received_features_equal_the_channel_calls(B, dtype, rng, path, dev):
    from fgnn_amd import _hip
    from fgnn_amd.tables import LdpcGraph
    gen = torch.Generator(device=dev).manual_seed(B)
    cw = path.encode(torch.randint(0, 2, (B, 48), device=dev, generator=gen))
    snr = torch.randint(0, 5, (B,), device=dev, generator=gen).float()
    sb = torch.randint(0, 6, (B,), device=dev, generator=gen).float()
    y, *want = path.channel_features(cw, snr, sb, 0.05, generator=gen, dtype=dtype, kernel_rng=(B, 7) if rng else None)
    for s in (snr, snr[:, None].expand(-1, 96).contiguous()):              # per word and the stored per-bit rows
        got = path.received_features(y, s, dtype)
        assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_received_features_kernel'
        for g, w in zip(got, want):
            assert g.dtype == dtype and g.shape == w.shape and torch.equal(g, w)
    # the host restatement of ldpc_dataset.py (the reference's numpy takes), on 64 words
    g = LdpcGraph()
    yh, sh = y.cpu().numpy(), snr.cpu().numpy()
    got = [t.cpu() for t in path.received_features(y, snr, dtype)]
    for b in range(min(B, 64)):
        for t, r in zip(got, g.features(yh[b], sh[b])):
            assert torch.equal(t[b], torch.from_numpy(r).to(dtype))


def test_received_features_read_per_bit_snr_rows(path, dev):
    y = torch.randn(5, 96, device=dev)
    snr = torch.arange(5 * 96, device=dev, dtype=torch.float32).reshape(5, 96) / 7
    node = path.received_features(y, snr)[0]
    assert torch.equal(node[:, 0, :, 0], y) and torch.equal(node[:, 1, :, 0], snr)
    with pytest.raises(ValueError):
        path.received_features(y, snr[:, :48])


# ---- 2. error counts ---------------------------------------------------------------------------------------------------------

def _count_case(B, seed):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, 48)).astype(np.float32)
    logits[rng.random((B, 48)) < 0.05] = 0.0
    logits[rng.random((B, 48)) < 0.05] = -0.0
    bits = rng.integers(0, 2, (B, 96)).astype(np.uint8)
    bits[rng.random((B, 96)) < 0.1] = 7                                    # any non-zero byte is a 1
    label = rng.integers(0, 2, (B, 96))
    label[rng.random(B) < 0.3] = 0                                         # some all-zero words
    snr = rng.choice(np.array([0, 1, 2, 3, 4, 2.5], np.float32), B)
    snr_rows = np.repeat(snr[:, None], 96, 1)
    snr_rows[:, 1:] += 0.5                                                 # only bit 0 classifies
    sb = rng.choice(np.array([0, 1, 2, 3, 4, 5, 2.7, 6], np.float32), B)
    return logits, bits, label, snr_rows, sb


@pytest.mark.parametrize('B', [1, 100, 4097, 70000])
@pytest.mark.parametrize('kind', ['f32', 'bf16', 'bytes'])
@pytest.mark.parametrize('label_dtype', ['int64', 'uint8'])
def test_error_counts_equal_the_restatement(B, kind, label_dtype, dev):
    from fgnn_amd import _hip
    from fgnn_amd.ldpc_eval import LdpcErrorCounts
    logits, bits, label, snr_rows, sb = _count_case(B, B)
    lab = torch.from_numpy(label.astype(np.int64 if label_dtype == 'int64' else np.uint8)).to(dev)
    snr_t, sb_t = torch.from_numpy(snr_rows).to(dev), torch.from_numpy(sb).to(dev)
    if kind == 'bytes':
        dec = torch.from_numpy(bits).to(dev)
        ref_dec, rkind = bits, 'bits'
    else:
        dec = torch.from_numpy(logits).to(dev, torch.float32 if kind == 'f32' else torch.bfloat16)
        ref_dec, rkind = dec.float().cpu().numpy(), 'logits'                 # (bf16: its own values; +-0 stay +-0)
    want = EO.error_counts(ref_dec, rkind, label, snr_rows[:, 0], sb)
    acc = LdpcErrorCounts(dev)
    add = acc.add_bits if kind == 'bytes' else acc.add_logits
    add(dec, lab, snr_t, sb_t)
    assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_error_counts_kernel'
    got = acc.result()['counts']
    assert np.array_equal(got, want), (got, want)
    # three calls accumulate to the one call on the concatenation; repeating gives identical counts
    acc.reset()
    cuts = [0, B // 3, (2 * B) // 3, B]
    for i, j in zip(cuts[:-1], cuts[1:]):
        add(dec[i:j], lab[i:j], snr_t[i:j], sb_t[i:j])
    assert np.array_equal(acc.result()['counts'], want)
    for i, j in zip(cuts[:-1], cuts[1:]):
        add(dec[i:j], lab[i:j], snr_t[i:j], sb_t[i:j])
    assert np.array_equal(acc.result()['counts'], 2 * want)


def test_error_counts_result_tables(dev):
    from fgnn_amd.ldpc_eval import LdpcErrorCounts
    logits, _, label, snr_rows, sb = _count_case(5000, 3)
    acc = LdpcErrorCounts(dev, snr_grid=(0, 1, 2, 3, 4, 7), sigma_grid=(0, 1, 2, 3, 4, 5))
    acc.add_logits(torch.from_numpy(logits).to(dev), torch.from_numpy(label).to(dev), torch.from_numpy(snr_rows[:, 0]).to(dev),
                   torch.from_numpy(sb).to(dev))
    r = acc.result()
    c = EO.error_counts(logits, 'logits', label, snr_rows[:, 0], sb, snr_grid=(0, 1, 2, 3, 4, 7))
    assert np.array_equal(r['counts'], c)
    cls = c[:-1].reshape(6, 6, 4)
    assert np.isnan(r['err_class'][5]).all() and np.isnan(r['fer_class'][5]).all()          # the empty SNR-7 row
    with np.errstate(invalid='ignore'):
        assert np.allclose(r['err_class'][:5], 1 - (cls[:5, :, 0] - cls[:5, :, 1]) / cls[:5, :, 0], rtol=0, atol=0)
    assert r['ber'] == 1 - int(c[-1, 0] - c[-1, 1]) / int(c[-1, 0]) and r['fer'] == c[-1, 3] / c[-1, 2]


# ---- 3. test sets ------------------------------------------------------------------------------------------------------------

def test_make_test_set_follows_the_generator(path, dev):
    num = 200
    d = path.make_test_set(num, seed=5)
    n = num * 30
    assert sorted(d) == ['gts', 'noizy_sg', 'sigma_b', 'snr_dbs', 'sp_error']
    assert d['noizy_sg'].dtype == torch.float32 and d['noizy_sg'].shape == (n, 96) and not d['noizy_sg'].is_cuda
    assert d['gts'].dtype == torch.int64 and d['gts'].shape == (n, 96)
    assert d['snr_dbs'].dtype == torch.float32 and d['snr_dbs'].shape == (n, 96)
    assert d['sigma_b'].dtype == torch.float32 and d['sigma_b'].shape == (n,)
    assert d['sp_error'].dtype == torch.float64 and d['sp_error'].shape == (5, 6)
    # sigma_b outer, SNR inner, num per class; constant SNR rows
    cls = torch.arange(30).repeat_interleave(num)
    assert torch.equal(d['sigma_b'], (cls // 5).float()) and torch.equal(d['snr_dbs'][:, 0], (cls % 5).float())
    assert torch.equal(d['snr_dbs'], d['snr_dbs'][:, :1].expand(-1, 96))
    # codewords
    assert torch.equal(path.encode(d['gts'][:, :48]).long().cpu(), d['gts'])
    # reproducible from its arguments
    e = path.make_test_set(num, seed=5)
    f = path.make_test_set(num, seed=6, baseline=False)
    assert all(torch.equal(d[k], e[k]) for k in d)
    assert not torch.equal(d['gts'], f['gts']) and not torch.equal(d['noizy_sg'], f['noizy_sg'])
    # the channel at sigma_b = 0: y - 2 gcx (t - 1/2) is unit white noise (>= 48 000 samples)
    z = d['sigma_b'] == 0
    gcx = torch.pow(10.0, d['snr_dbs'][z].double() / 20)
    r = (d['noizy_sg'][z].double() - 2 * gcx * (d['gts'][z].double() - 0.5)).flatten()
    assert r.numel() >= 48000
    print('residual mean %.4f var %.4f over %d samples' % (float(r.mean()), float(r.var()), r.numel()))
    assert abs(float(r.mean())) < 0.02 and abs(float(r.var()) - 1) < 0.02
    # the sum-product table: the decoder's mean message-bit error per class, on the returned words
    y, snr = d['noizy_sg'].to(dev), d['snr_dbs'][:, 0].to(dev)
    x = path.decode(path.bit_prior(y, snr), loops=100)[0].cpu().numpy()
    c = EO.error_counts(x, 'bits', d['gts'].numpy(), d['snr_dbs'][:, 0].numpy(), d['sigma_b'].numpy())
    tot = c[:-1, 0].reshape(5, 6)
    want = 1 - (tot - c[:-1, 1].reshape(5, 6)) / tot                      # 1 - acc_cnt / acc_tot, as the reference forms it
    assert np.array_equal(d['sp_error'].numpy(), want)
    print('sum-product table\n', d['sp_error'])
    assert d['sp_error'][4, 0] < d['sp_error'][0, 0]


# ---- 4. round trip -----------------------------------------------------------------------------------------------------------

def test_written_test_set_evaluates_like_the_dict(path, model, tmp_path):
    from fgnn_amd.ldpc_eval import evaluate
    p = str(tmp_path / 'ldpc_test.pt')
    sp = path.write_test_set(p, 10, seed=3)
    saved = torch.load(p)
    assert sorted(saved) == ['gts', 'noizy_sg', 'sigma_b', 'snr_dbs'] and sp.shape == (5, 6)
    d = path.make_test_set(10, seed=3, baseline=False)
    assert all(torch.equal(saved[k], d[k]) for k in saved)
    a, b = evaluate(model, p, batch_size=128), evaluate(model, d, batch_size=128)
    assert np.array_equal(a['counts'], b['counts']) and a['counts'][-1, 2] == 300
    model.train()
    c = evaluate(model, d, batch_size=128, baseline=True)
    assert model.training                                                  # the flag is restored
    model.eval()
    assert np.array_equal(c['counts'], a['counts'])
    assert np.array_equal(c['baseline']['err_class'], sp.numpy())


# ---- 5. against the reference's loop ------------------------------------------------------------------------------------------

def test_evaluate_counts_what_the_reference_loop_counts(path, model, dev):
    from fgnn_amd.ldpc_eval import evaluate
    from fgnn_amd.tables import LdpcGraph
    d = path.make_test_set(40, seed=9, baseline=False)
    n = d['noizy_sg'].shape[0]
    g = LdpcGraph()
    want = np.zeros((31, 4), np.int64)
    near = 0
    i1 = path.nn_idx_f2v.unsqueeze(0)
    i2 = path.nn_idx_v2f.unsqueeze(0)
    for i in range(0, n, 100):                     # the reference: Codes items (host numpy features), batches of 100
        j = min(n, i + 100)
        feats = [g.features(d['noizy_sg'][b].numpy(), 0.0) for b in range(i, j)]
        node, hop, e1, e2 = (torch.from_numpy(np.stack([f[k] for f in feats])).to(dev) for k in range(4))
        node[:, 1, :, 0] = d['snr_dbs'][i:j].to(dev)                        # the stored per-bit SNR rows
        with torch.no_grad():
            logits, _ = model(node, hop, i1.expand(j - i, -1, -1), i2.expand(j - i, -1, -1), e1, e2)
        lg = logits.float().cpu().numpy()
        near += int((np.abs(lg) <= 1e-5).sum())
        want += EO.error_counts(lg, 'logits', d['gts'][i:j].numpy(), d['snr_dbs'][i:j, 0].numpy(), d['sigma_b'][i:j].numpy())
    print('logits within 1e-5 of zero:', near)
    got = evaluate(model, d, batch_size=512)['counts']
    assert np.abs(got - want).max() <= near, (got, want)
    a, b = evaluate(model, d, batch_size=100)['counts'], evaluate(model, d, batch_size=4096)['counts']
    assert np.abs(a - b).max() <= near
    assert want[-1, 2] == n and want[:-1, 2].sum() == n


def test_evaluate_bf16(path, model, small_set):
    from fgnn_amd.ldpc_eval import evaluate
    r = evaluate(model, small_set, batch_size=64, dtype=torch.bfloat16)
    assert r['counts'][-1, 2] == 120 and r['counts'][-1, 0] == 120 * 48 and 0 <= r['ber'] <= 1


# ---- 6. command line ---------------------------------------------------------------------------------------------------------

def test_command_line_prints_what_evaluate_returns(model, tmp_path, dev):
    from fgnn_amd.ldpc_eval import evaluate
    ts, ck = str(tmp_path / 'set.pt'), str(tmp_path / 'ckpt.pt')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
    run = lambda *a: subprocess.run([sys.executable, '-m', 'fgnn_amd.ldpc_eval'] + list(a), capture_output=True, text=True, env=env,
                                    cwd=str(tmp_path), timeout=600)
    r = run('--make_test_set', ts, '--num', '6', '--seed', '2')
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'tensor(' in r.stdout and os.path.exists(ts)
    torch.save({'model_state_dict': model.state_dict()}, ck)
    r = run('--test_path', ts, '--model_path', ck, '--batch_size', '64', '--baseline')
    assert r.returncode == 0, r.stderr[-3000:]
    res = evaluate(model, ts, batch_size=64, baseline=True)
    want = '%s\n%s\n%s\n' % (res['ber'], torch.FloatTensor(res['err_class']), torch.FloatTensor(res['baseline']['err_class']))
    print(r.stdout)
    assert r.stdout.endswith(want), (r.stdout, want)
