"""GPU: the layers that take an ``LdpcCode`` — the W-word encoder and sampler (include/fgnn_hip_ldpc_code.h; csrc/ldpc_code.hip) against
the oracle and their numpy restatement (tests/ldpc_code_oracle.py), the unchanged channel / received-feature / decoder entry points at
new shapes, ``LDPCModel.for_code`` against the oracle's parts, and the training / evaluation loop on a code of its own.  The reference
is locked to 96.3.963, so these are properties plus the oracle, not reference vectors."""
import contextlib
import ctypes
import functools
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fgnn_oracle as O
import helpers as H
import ldpc_code_oracle as CO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'factor-graph-neural-network_amd')
CODES = {'G12': (12, 3, 4, 0), 'G24': (24, 3, 6, 0), 'G132': (132, 3, 6, 0), 'G204': (204, 3, 6, 0)}
SEEDS = [(0, 0), (2 ** 64 - 59, 2 ** 33 + 1)]


def _code(name):
    from fgnn_amd.ldpc_code import LdpcCode
    return LdpcCode.builtin() if name == 'builtin' else CO.gallager(*CODES[name])


@functools.lru_cache(maxsize=None)
def _path(name):
    from fgnn_amd.datapath import LdpcDataPath
    return LdpcDataPath(torch.device('cuda:0'), _code(name))


@pytest.fixture
def paths(dev):
    return _path


@functools.lru_cache(maxsize=None)
def _restated(name, B, seed, step):
    out = CO.sample_batch(_code(name).G, B, seed, step)
    for a in out:
        a.setflags(write=False)
    return out


def _pack(G):
    """Rows of a 0/1 matrix [P, K] -> uint64 [P, ceil(K / 64)], bit c of a row in bit c % 64 of word c // 64 (restated here)."""
    P, K = G.shape
    W = -(-K // 64)
    out = np.zeros((P, W), np.uint64)
    for r in range(P):
        for c in np.nonzero(G[r])[0]:
            out[r, c // 64] |= np.uint64(1) << np.uint64(c % 64)
    return out


# ---- 1. the encoder -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [1, 65, 130])
@pytest.mark.parametrize('K, P', [(1, 1), (5, 7), (63, 64), (64, 65), (65, 24), (128, 3), (129, 64), (1000, 24),
                                  (513, 511)])        # the last: the largest LDS footprint, (64 + P) W words = 41 400 bytes
def test_encoder_words_bit_exact_against_the_oracle(K, P, B, dev):
    from fgnn_amd import _hip
    rng = np.random.default_rng(1000 * K + P)
    G = rng.integers(0, 2, (P, K)).astype(np.uint8)
    s = rng.integers(0, 2, (B, K)).astype(np.uint8)
    W = -(-K // 64)
    gw = torch.from_numpy(_pack(G).view(np.int64)).to(dev)
    cw = torch.full((B + 1, K + P), 7, dtype=torch.uint8, device=dev)              # one guard row behind the batch
    _hip.call('fgnn_ldpc_encode_words', torch.from_numpy(s).to(dev), gw, B, K, P, W, cw)
    assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_encode_words_kernel'
    got = cw.cpu().numpy()
    assert np.array_equal(got[:B], O.ldpc_encode(G, s)) and (got[B] == 7).all()
    # only bit 0 of a message byte counts, as in the one-word encoder
    _hip.call('fgnn_ldpc_encode_words', torch.from_numpy(s | 0xFE).to(dev), gw, B, K, P, W, cw)
    assert np.array_equal(cw.cpu().numpy()[:B], O.ldpc_encode(G, s))


@pytest.mark.parametrize('offset', [0, 1, 2])
def test_encoder_words_equals_the_one_word_encoder_on_the_builtin_code(offset, paths, dev):
    """... also where the output does not start on a 4-byte boundary (the byte-store path)."""
    from fgnn_amd import _hip
    path = paths('builtin')
    s = torch.randint(0, 2, (130, 48), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(dev)
    old = path.encode(s)
    assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_encode_kernel'           # the default path keeps its kernel
    flat = torch.zeros(130 * 96 + 8, dtype=torch.uint8, device=dev)
    new = flat[offset:offset + 130 * 96].view(130, 96)
    _hip.call('fgnn_ldpc_encode_words', s, path.gmask, 130, 48, 48, 1, new)
    assert torch.equal(new, old) and not flat[:offset].any() and not flat[offset + 130 * 96:].any()
    assert np.array_equal(old.cpu().numpy(), O.ldpc_encode(path.code.G, s.cpu().numpy()))


@pytest.mark.parametrize('name', ['G12', 'G132', 'G204'])
def test_path_encode_gives_codewords_of_the_code(name, paths, dev):
    path = paths(name)
    c = path.code
    s = np.random.default_rng(3).integers(0, 2, (70, c.K)).astype(np.uint8)
    cw = path.encode(torch.from_numpy(s)).cpu().numpy()
    assert np.array_equal(cw, O.ldpc_encode(c.G, s)) and not ((cw.astype(np.int64) @ c.H.T.astype(np.int64)) % 2).any()
    with pytest.raises(ValueError):
        path.encode(torch.zeros(4, c.K + 1, dtype=torch.uint8))
    assert path.encode(torch.zeros(0, c.K, dtype=torch.uint8)).shape == (0, c.n_var)


# ---- 2. the sampler -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed, step', SEEDS, ids=['seed0_step0', 'seed64_step2p33'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('B', [1, 3, 65])
@pytest.mark.parametrize('name', ['G12', 'G132', 'G204'])
def test_sampler_equals_its_restatement_and_the_kernels_it_is_made_of(name, B, dtype, seed, step, paths):
    from fgnn_amd import _hip
    path = paths(name)
    c = path.code
    N, M, K = c.n_var, c.n_chk, c.K
    d = path.sample_rng(B, seed=seed, step=step, dtype=dtype)
    assert _hip.lib().fgnn_last_kernel().decode() == ('ldpc_sample_words_kernel' if K > 64 else 'ldpc_features_kernel<rng, draw>')
    cw_ref, snr_ref, sb_ref, y_ref = _restated(name, B, seed, step)
    assert d.cw.dtype == torch.uint8 and np.array_equal(d.cw.cpu().numpy(), cw_ref)
    assert d.snr_db.dtype == torch.float32 and np.array_equal(d.snr_db.cpu().numpy(), snr_ref)
    assert d.sigma_b.dtype == torch.float32 and np.array_equal(d.sigma_b.cpu().numpy(), sb_ref)
    assert torch.equal(d.cw, path.encode(d.cw[:, :K]))
    assert d.label.dtype == torch.float32 and d.label.shape == (B, K) and torch.equal(d.label, d.cw[:, :K].float())
    y, node, hop, e1, e2 = path.channel_features(d.cw, d.snr_db, d.sigma_b, 0.05, dtype=dtype, kernel_rng=(seed, step))
    for what, got, want in (('y', d.y, y), ('node', d.node_feature, node), ('hop', d.hop_feature, hop), ('ef_f2v', d.efeature_f2v, e1),
                            ('ef_v2f', d.efeature_v2f, e2)):
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), what
    assert d.node_feature.shape == (B, 2, N, 1) and d.hop_feature.shape == (B, c.dc, M, 1) and d.node_feature.dtype == dtype
    assert d.efeature_f2v.shape == (B, c.dc + 1, N, c.dv) and d.efeature_v2f.shape == (B, c.dc + 1, M, c.dc)
    err = np.abs(d.y.cpu().numpy() - y_ref).max()
    print(name, B, 'y err', err, 'of', np.abs(y_ref).max())
    assert err <= 2e-5 * np.abs(y_ref).max(), err
    assert d.nn_idx_f2v.shape == (B, N, c.dv) and d.nn_idx_v2f.shape == (B, M, c.dc) and d.nn_idx_f2v.dtype == torch.int64
    assert np.array_equal(d.nn_idx_f2v[0].cpu().numpy(), c.var_to_factors) and np.array_equal(d.nn_idx_v2f[0].cpu().numpy(), c.factor_to_vars)
    # received features: the existing identity at this shape, per-word and per-bit SNR
    for snr_arg in (d.snr_db, d.snr_db[:, None].expand(-1, N)):
        for what, got, want in zip(('node', 'hop', 'ef_f2v', 'ef_v2f'), path.received_features(d.y, snr_arg, dtype), (node, hop, e1, e2)):
            assert torch.equal(got, want), what


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', ['G132', 'G204'])
def test_sampler_is_cut_invariant_and_writes_in_place(name, dtype, paths):
    from fgnn_amd import _hip
    path = paths(name)
    seed, step = SEEDS[1]
    a = path.sample_rng(65, seed=seed, step=step, dtype=dtype)
    b = path.sample_rng(16, seed=seed, step=step, dtype=dtype)
    for what, x, y in zip(a._fields, a, b):
        assert torch.equal(x[:16], y), what
    ptrs, was = [t.data_ptr() for t in a], [t.clone() for t in a]
    again = path.sample_rng(65, seed=seed, step=step + 1, dtype=dtype, out=a)
    assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_sample_words_kernel'     # ONE launch, and it is the sampler's
    assert again is a and [t.data_ptr() for t in again] == ptrs
    fresh = path.sample_rng(65, seed=seed, step=step + 1, dtype=dtype)
    for what, x, y, old in zip(a._fields, a, fresh, was):
        assert torch.equal(x, y), what
        if what not in ('nn_idx_f2v', 'nn_idx_v2f'):
            assert not torch.equal(x, old), what
    same = float((a.label == was[6]).float().mean())
    assert 0.4 <= same <= 0.6, same                                                  # every message word is drawn anew, not only word 0
    with pytest.raises(ValueError):
        path.sample_rng(64, seed=seed, step=step, dtype=dtype, out=a)
    assert path.sample_rng(0, dtype=dtype).label.shape == (0, path.K)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_builtin_sampler_is_unchanged_and_the_words_sampler_draws_its_bits(dtype, paths, dev):
    """The default path: the one-word kernel and the bits of its restatement (tests/ldpc_train_oracle.py).  Through the C ABI the
    W-word sampler, handed the built-in code, writes the same eleven arrays."""
    import ldpc_train_oracle as TR
    from fgnn_amd import _hip
    from fgnn_amd.datapath import LdpcDataPath
    for path in (paths('builtin'), LdpcDataPath(dev)):
        assert path.code.is_default and path.gmask.shape == (48,) and (path.K, path.P) == (48, 48)
    seed, step = SEEDS[1]
    d = path.sample_rng(65, seed=seed, step=step, dtype=dtype)
    assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_features_kernel<rng, draw>'
    cw_ref, snr_ref, sb_ref, _ = TR.sample_batch(H.load('ldpc_datapath.npz')['G'], 65, seed, step)
    assert np.array_equal(d.cw.cpu().numpy(), cw_ref) and np.array_equal(d.snr_db.cpu().numpy(), snr_ref)
    assert np.array_equal(d.sigma_b.cpu().numpy(), sb_ref)
    w = LdpcDataPath(dev).sample_rng(65, seed=1, step=1, dtype=dtype)                # buffers of the right shapes, other contents
    farr = lambda c: (ctypes.c_float * len(c))(*[float(v) for v in c])
    _hip.call('fgnn_ldpc_sample_rng_words', seed, step, farr(path.snr_db_choices), 5, farr(path.sigma_b_choices), 6, 0.05, path.gmask,
              path.var_to_factors, path.factor_to_vars, 65, 48, 48, 1, 48, 3, 6, _hip.dtype_code(w.node_feature), w.node_feature,
              w.hop_feature, w.efeature_f2v, w.efeature_v2f, w.snr_db, w.sigma_b, w.cw, w.label, w.y)
    assert _hip.lib().fgnn_last_kernel().decode() == 'ldpc_sample_words_kernel'
    for what, x, y in zip(d._fields, d, w):
        assert torch.equal(x, y), what


def test_sampler_at_1024_variables(dev):
    """The largest row the feature kernels take: four passes of the channel loop, the classes beside a full ``ys``."""
    from fgnn_amd.datapath import LdpcDataPath
    c = CO.gallager(1024, 3, 8, 0)
    assert c.n_var == 1024 and c.W == 11
    path = LdpcDataPath(dev, c)
    seed, step = SEEDS[1]
    d = path.sample_rng(2, seed=seed, step=step, dtype=torch.float32)
    cw_ref, snr_ref, sb_ref, y_ref = CO.sample_batch(c.G, 2, seed, step)
    assert np.array_equal(d.cw.cpu().numpy(), cw_ref) and not ((cw_ref.astype(np.int64) @ c.H.T.astype(np.int64)) % 2).any()
    assert np.array_equal(d.snr_db.cpu().numpy(), snr_ref) and np.array_equal(d.sigma_b.cpu().numpy(), sb_ref)
    err = np.abs(d.y.cpu().numpy() - y_ref).max()
    print('N = 1024 y err', err, 'of', np.abs(y_ref).max())
    assert err <= 2e-5 * np.abs(y_ref).max(), err
    assert torch.equal(d.node_feature[:, 0, :, 0], d.y) and torch.equal(d.node_feature[:, 1, :, 0], d.snr_db[:, None].expand(-1, 1024))
    assert torch.equal(d.hop_feature[:, :, :, 0].permute(0, 2, 1), d.y[:, path.nn_idx_v2f])
    assert torch.equal(d.cw, path.encode(d.cw[:, :c.K]))
    with pytest.raises(ValueError, match='1024'):
        path.decode(path.bit_prior(d.y, d.snr_db))                                   # 3072 edges: beyond the decoder, not the data path


# ---- 4. the decoder -------------------------------------------------------------------------------------------------------------

def test_sum_product_decoder_on_g132(paths, dev):
    path = paths('G132')
    c = path.code
    B = 64
    s = np.random.default_rng(4).integers(0, 2, (B, c.K)).astype(np.uint8)
    cw = path.encode(torch.from_numpy(s))
    snr = torch.full((B,), 4.0)
    y = path.channel_features(cw, snr, torch.zeros(B), 0.05, kernel_rng=(4, 0))[0].cpu().numpy()
    bias = O.ldpc_bit_prior(y, snr.numpy())
    x, viol, iters = (t.cpu().numpy() for t in path.decode(torch.from_numpy(bias), loops=50))
    for i in range(0, B, 11):                                                        # 6 words through the (pure-Python) oracle
        xo, _, vo, io = O.ldpc_sum_product(c.nlist, c.n_chk, bias[i], loops=50)
        assert np.array_equal(x[i], xo) and viol[i] == vo and iters[i] == io, i
    syn = ((x.astype(np.int64) @ c.H.T.astype(np.int64)) % 2).sum(1)
    assert np.array_equal(syn, viol)
    cwn = cw.cpu().numpy()
    raw, dec = int(((y > 0) != (cwn > 0)).sum()), int((x != cwn).sum())
    print('G132 at 4 dB: %d of %d words reach zero syndrome, %d bit errors after decoding against %d of hard decisions on y, '
          'iterations %s' % ((viol == 0).sum(), B, dec, raw, np.bincount(iters).tolist()))
    assert (viol == 0).sum() >= B // 2 and dec < raw


# ---- 5. the model ---------------------------------------------------------------------------------------------------------------

def _model_and_batch(name, dev, dtype=torch.float32):
    from fgnn_amd.ldpc import LDPCModel
    path = _path(name)
    m = LDPCModel.for_code(path.code)
    m.load_state_dict(H.fill_state_dict(m.state_dict()))
    return m.to(dev), path, path.sample_rng(4, seed=6, step=0, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _unreached_by_the_default_model(dev):
    """Names of the trainable parameters of ``LDPCModel(2, 6, 4)`` that one train-mode backward on a built-in batch leaves without a gradient."""
    from fgnn_amd.ldpc import LDPCModel, decoding_loss
    m = LDPCModel(2, 6, 4)
    m.load_state_dict(H.fill_state_dict(m.state_dict()))
    m = m.to(dev).train()
    d = _path('builtin').sample_rng(4, seed=6, step=0, dtype=torch.float32)
    logits, snr = m(*d[:6])
    decoding_loss(logits, snr, d.label, d.sigma_b, 0.1).backward()
    return frozenset(k for k, p in m.named_parameters() if p.requires_grad and p.grad is None)


@pytest.mark.parametrize('mode', ['eval', 'train'])
@pytest.mark.parametrize('name', ['G24', 'G132'])
def test_model_for_code_against_the_oracle(name, mode, dev):
    m, path, d = _model_and_batch(name, dev)
    c = path.code
    train = mode == 'train'
    m.train(train)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with contextlib.nullcontext() if train else torch.no_grad():
        logits, snr = m(*d[:6])
    assert logits.shape == (4, c.K) and snr.shape == (4, 1)
    with torch.no_grad():
        lo, so = CO.ldpc_model(sd, c.K, *[t.cpu().contiguous() for t in d[:6]], training=train)
    el, es = H.rel_err(logits, lo), H.rel_err(snr, so)
    print(name, mode, 'logit err %.3e snr head err %.3e (logit range %.3g)' % (el, es, float(lo.abs().max())))
    assert el <= 1e-4 and es <= 1e-4
    if train:
        worst = 0.0
        for k, v in m.state_dict().items():
            if k.endswith(('running_var', 'running_mean')):
                worst = max(worst, H.rel_err(v, sd[k]))
            elif k.endswith('num_batches_tracked'):
                assert int(v) == 1, k                                                # (the oracle's batch_norm keeps no count)
        print(name, 'running statistics vs oracle: worst %.2e' % worst)
        assert worst <= 1e-4
        from fgnn_amd.ldpc import decoding_loss
        decoding_loss(logits, snr, d.label, d.sigma_b, 0.1).backward()
        # every parameter the loss reaches has a finite gradient; the ones it does not reach (an InstanceNorm over the hyper-factor's
        # single node gives zeros whatever its map's weights) are those of the default model on the built-in code, by name
        grads = {k: p.grad for k, p in m.named_parameters() if p.requires_grad}
        unreached = {k for k, g in grads.items() if g is None}
        assert unreached == _unreached_by_the_default_model(dev)
        # ... pinned by name: the hyper-factor's f2f map of every layer is among them (blocks.iid_mapping_in returns zeros for one node),
        # and nothing outside the modules whose output the loss cannot depend on — that map, and the last layer's parity-factor
        # state, which neither the classifier (variables) nor the regressor (hyper-factor) reads
        assert unreached >= {'main.f2f_%d_1.main.0.%s' % (L, w) for L in range(8) for w in ('weight', 'bias')}
        allowed = tuple('main.f2f_%d_1.' % L for L in range(8)) + ('main.v2f_7_0.', 'main.f2f_7_0.')
        assert all(k.startswith(allowed) for k in unreached), sorted(k for k in unreached if not k.startswith(allowed))
        print(name, 'parameters without a gradient:', len(unreached), 'of', len(grads))
        assert sum(g is not None for g in grads.values()) > 100 and all(torch.isfinite(g).all() for g in grads.values() if g is not None)


@pytest.mark.parametrize('name', ['G24', 'G132'])
def test_model_for_code_in_bf16(name, dev):
    """(G24: a 3-6 code small enough for the table-driven bf16 operator kernels; G132: beyond them and beyond the hyper-factor kernels.)
    bf16 activations under autocast against the f32 oracle on the bf16-rounded inputs, as tests/test_parity_pins_gpu.py judges the
    benched model: the constructor's own initialisation, running statistics from three train-mode batches, then eval; logits and SNR
    head within that test's 2e-2 (of the logit range / of max(1, |head|))."""
    from fgnn_amd.ldpc import LDPCModel
    path = _path(name)
    c = path.code
    torch.manual_seed(3)
    m = LDPCModel.for_code(c).to(dev).train()
    with torch.no_grad():
        for i in range(3):
            m(*path.sample_rng(256, seed=50 + i, dtype=torch.float32)[:6])
    m.eval()
    d = path.sample_rng(4, seed=6, step=0, dtype=torch.bfloat16)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        logits, snr = m(*d[:6])
    assert torch.isfinite(logits.float()).all() and torch.isfinite(snr.float()).all()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    o_in = [t.cpu().contiguous() for t in d[:6]]
    with torch.no_grad():
        lo, so = CO.ldpc_model(sd, c.K, *[t.float() if t.is_floating_point() else t for t in o_in], training=False)
    rng = float(lo.abs().max())
    err = float((logits.float().cpu() - lo).abs().max()) / rng
    serr = float((snr.float().cpu() - so).abs().max()) / max(1.0, float(so.abs().max()))
    print('bf16 LDPCModel.for_code(%s) vs f32 oracle: logit err %.3e of range %.3g, snr head err %.2e' % (name, err, rng, serr))
    assert err <= 2e-2 and serr <= 2e-2


# ---- 6. the loop ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def g24_runs(dev, tmp_path_factory):
    from fgnn_amd import ldpc_train
    out = {}
    for which, graph in (('eager', False), ('graphed', True)):
        d = str(tmp_path_factory.mktemp('g24_' + which))
        with contextlib.redirect_stdout(io.StringIO()):
            out[which] = ldpc_train.train(n_epochs=1, steps_per_epoch=4, batch_size=8, log_every=2, graph=graph, out_dir=d, device=dev,
                                          code=_code('G24'))
    return out


def test_loop_at_a_batch_with_merged_gradient_paths_graphed_like_eager(dev, tmp_path):
    """B = 64: B·N = 1536 rows, above the 1024 at which the backward's merged fan-gradient / weight-gradient paths start."""
    from fgnn_amd import ldpc_train
    out = {}
    for which, graph in (('eager', False), ('graphed', True)):
        with contextlib.redirect_stdout(io.StringIO()):
            out[which] = ldpc_train.train(n_epochs=1, steps_per_epoch=4, batch_size=64, log_every=2, graph=graph, out_dir=str(tmp_path / which),
                                          device=dev, code=_code('G24'))
    e, g = out['eager'], out['graphed']
    print('eager', e['losses'], 'graphed', g['losses'])
    assert g['graphed'] and not e['graphed'] and g['losses'][:3] == e['losses'][:3]
    assert all(np.isfinite(e['losses'])) and len(e['losses']) == 4


def test_trainer_refuses_a_code_outside_its_class(dev, tmp_path):
    from fgnn_amd import ldpc_train
    with pytest.raises(ValueError, match='dv = 3, dc = 6 and N <= 96'):
        ldpc_train.train(n_epochs=1, steps_per_epoch=1, batch_size=8, out_dir=str(tmp_path), device=dev, code=_code('G132'))


def test_loop_trains_a_code_of_its_own_graphed_like_eager(g24_runs):
    e, g = g24_runs['eager'], g24_runs['graphed']
    print('eager', e['losses'], 'graphed', g['losses'])
    assert g['graphed'] and not e['graphed']
    assert g['losses'][:3] == e['losses'][:3]                                        # test_graphed_loop_starts_like_the_eager_one's
    for r in (e, g):
        assert r['steps'] == r['gcnt'] == 4 and len(r['losses']) == 4 and all(np.isfinite(r['losses'])) and 0.0 <= r['acc'] <= 1.0


def test_checkpoint_carries_its_code_and_evaluates_on_it(g24_runs, paths, dev):
    from fgnn_amd import ldpc_eval, ldpc_train
    c = _code('G24')
    where = g24_runs['graphed']['checkpoint']
    ck = torch.load(where, map_location='cpu', weights_only=True)
    assert set(ck) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt', 'code'}
    assert int(ck['code']['n_var']) == 24 and torch.equal(ck['code']['var_to_factors'], torch.from_numpy(c.var_to_factors.copy()))
    ts = paths('G24').make_test_set(num=2)
    n = 2 * 30
    assert ts['noizy_sg'].shape == (n, 24) and ts['gts'].shape == (n, 24) and ts['snr_dbs'].shape == (n, 24) and ts['sp_error'].shape == (5, 6)
    assert not ((ts['gts'].numpy() @ c.H.T.astype(np.int64)) % 2).any()
    res = ldpc_eval.evaluate(where, ts, dtype=torch.bfloat16, baseline=True, code=c)
    assert res['err_class'].shape == (5, 6) and res['counts'][-1][0] == n * c.K and 0.0 <= res['ber'] <= 1.0
    assert res['baseline']['counts'][-1][0] == n * c.K
    assert np.array_equal(res['baseline']['err_class'], ts['sp_error'].numpy())     # the same decoder on the same words (loops = 100)
    model = ldpc_eval.load_model(where, c, device=dev)
    again = ldpc_eval.evaluate(model, ts, dtype=torch.bfloat16, code=c)
    assert again['ber'] == res['ber'] and np.array_equal(again['counts'], res['counts'])
    with pytest.raises(ValueError, match='trained for a code with'):
        ldpc_eval.evaluate(where, ts)                                                # the default code
    with pytest.raises(ValueError, match='trained for'):
        ldpc_eval.load_model(where, CO.gallager(24, 3, 6, 1))
    with pytest.raises(ValueError, match='trained for'):
        ldpc_train.train(n_epochs=2, steps_per_epoch=1, batch_size=8, model_path=where, device=dev)
    with pytest.raises(ValueError, match='pass the code the model was built for'):
        ldpc_eval.evaluate(model, ts)


def test_command_line_trains_a_gallager_code(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG] + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, '-m', 'fgnn_amd.ldpc_train', '--code', 'gallager:24,3,6,0', '--n_epochs', '1', '--batch_size', '8',
                        '--steps_per_epoch', '2', '--json', '--out_dir', str(tmp_path)], capture_output=True, text=True, env=env,
                       cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res['steps'] == 2 and res['gcnt'] == 2
    assert res['checkpoint'] == os.path.join(str(tmp_path), 'FactorNN_nn_factor_epoches_1_snr_None.pt') and os.path.exists(res['checkpoint'])
    ck = torch.load(res['checkpoint'], map_location='cpu', weights_only=True)
    assert int(ck['code']['n_var']) == 24 and int(ck['code']['dc']) == 6
