"""GPU: the learned min-sum LDPC decoder (csrc/ldpc_nms.hip; fgnn_amd/ldpc_nms.py, ldpc_nms_train.py, ldpc_eval's learned-min-sum spec)
against the existing LLR-domain kernel and the restatement tests/ldpc_nms_oracle.py.

Inputs are tests/test_ldpc_nms.py's (``words``, ``weights``, ``g_totals``: the received words of tests/test_ldpc_llr_gpu.py, B = 67 at its
SNR_DB; g1024 with B = 5 and n_iter = 3), and so are the yardstick and its measurement: ``D``, per output tensor the largest
|g_f32 - g_f64| / max |g_f64| between the restatement's own two precisions, g_alpha 2.967e-07, g_beta 3.674e-07, g_llr 1.750e-07,
measured on the CPU by ``test_ldpc_nms.restatement_error`` over every (code, share) of this file.  The backward's bound is 4 d per
tensor, as SP_BOUND is formed: the device adds the words and the edges in another order than numpy does, errors of the size that
separate the two precisions.  Only words whose f32 and f64 records agree in every field are given to the device (``kept``; on these
inputs that is every word, asserted on the CPU).

Forward: every operation is an IEEE f32 add, subtract, multiply, maximum or compare in a fixed order, so the decode mode with constant
weights equals fgnn_ldpc_decode_llr's flooding min-sum / offset min-sum bit for bit, and the train mode's totals equal the f32
restatement bit for bit."""
import numpy as np
import pytest
import torch

import ldpc_nms_oracle as NO
from ldpc_decoder_cases import ZeroLogits, make_paths, received
import test_ldpc_llr_gpu as LG
import test_ldpc_nms as NC

pytestmark = pytest.mark.gpu

CODES, SHARES, N_ITER = NC.CODES, NC.SHARES, NC.N_ITER
BOUND = {k: 4 * d for k, d in NC.D.items()}


paths = pytest.fixture(scope='module', name='paths')(make_paths)


def cuda(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()       # (a copy in C order: a[:, mask] comes with strides of its own)


def module(name, share, alpha, beta):
    """A ``LearnedMinSum`` on the device holding the given weights ([n_iter, W] arrays, or two constants with ``share`` + n_iter)."""
    from fgnn_amd.ldpc_nms import LearnedMinSum
    dec = LearnedMinSum(LG.case(name)[0], alpha.shape[0], share).cuda()
    with torch.no_grad():
        dec.alpha.copy_(cuda(alpha))
        dec.beta.copy_(cuda(beta))
    return dec


def train_forward(dec, llr):
    """The train mode through the C ABI with every optional output: (totals, record, x, viol, iters) as device tensors."""
    from fgnn_amd import _hip
    llr = llr if isinstance(llr, torch.Tensor) else cuda(llr)
    B, N, M, E = llr.shape[0], dec.N, dec.M, dec.E
    nbytes = int(_hip.invoke('fgnn_ldpc_nms_record_bytes', B, N, M, E, dec.n_iter))
    totals = torch.empty((dec.n_iter, B, N), device='cuda')
    record = torch.empty((nbytes,), dtype=torch.uint8, device='cuda')
    x = torch.empty((B, N), dtype=torch.uint8, device='cuda')
    viol, iters = torch.empty((B,), dtype=torch.int32, device='cuda'), torch.empty((B,), dtype=torch.int32, device='cuda')
    _hip.call('fgnn_ldpc_nms_forward', llr, llr.stride(0), dec.col_ptr, dec.row_ptr, dec.row_edge, dec.row_var, dec.alpha.detach(),
              dec.beta.detach(), B, N, M, E, dec.n_iter, NO.SHARES.index(dec.share), 0, x, None, viol, iters, totals, record, nbytes)
    return totals, record, x, viol, iters


def device_backward(dec, llr, g, want_llr=True):
    """Forward (train mode) and backward through the raw launches: (g_alpha, g_beta, g_llr) as numpy arrays."""
    from fgnn_amd.ldpc_nms import nms_backward_raw, nms_forward_raw
    llr, g = cuda(llr), cuda(g)
    tables, sizes, share = (dec.col_ptr, dec.row_ptr, dec.row_edge, dec.row_var), (dec.N, dec.M, dec.E), NO.SHARES.index(dec.share)
    alpha, beta = dec.alpha.detach(), dec.beta.detach()
    _, record = nms_forward_raw(llr, tables, sizes, alpha, beta, dec.n_iter, share)
    out = nms_backward_raw(g, llr, tables, sizes, alpha, beta, record, dec.n_iter, share, want_llr)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@pytest.mark.parametrize('name', CODES)
def test_decode_mode_with_constant_weights_is_the_llr_kernel_bit_for_bit(paths, name):
    llr = cuda(LG.case(name)[3])
    it = LG.MS_ITERS
    for algorithm, alpha, beta in (('min-sum', 0.8125, 0.0), ('offset-min-sum', 1.0, 0.5)):
        dec = module(name, 'iteration', np.full((it, 1), alpha, np.float32), np.full((it, 1), beta, np.float32))
        for rows in (slice(None), slice(0, 1)):                                # B = 67, B = 1
            want = paths(name).decode_llr(llr[rows], algorithm, 'flooding', max_iter=it, alpha=0.8125, beta=0.5, want_posteriors=True)
            got = dec.decode(llr[rows], want_posteriors=True)
            for g, w in zip(got[:3], want[:3]):
                assert g.dtype == w.dtype and torch.equal(g, w)
            post, ref = got[3].cpu().numpy(), want[3].cpu().numpy()
            nan = np.isnan(ref)                                                 # NaN places are compared as places
            assert np.array_equal(np.isnan(post), nan) and np.array_equal(LG.bits(post)[~nan], LG.bits(ref)[~nan])
        assert dec.decode(llr)[0].shape == llr.shape and len(dec.decode(llr)) == 3
        assert dec.decode(torch.zeros(0, llr.shape[1], device='cuda'))[0].shape == (0, llr.shape[1])       # B = 0: no launch


@pytest.mark.parametrize('share', SHARES)
@pytest.mark.parametrize('name', CODES)
def test_train_mode_equals_the_restatement_bit_for_bit(name, share):
    alpha, beta = NC.weights(name, share)
    want = NC.restated(name, share)
    dec = module(name, share, alpha, beta)
    totals, _, x, viol, iters = train_forward(dec, NC.words(name))
    totals = totals.cpu().numpy()
    assert np.array_equal(LG.bits(totals), LG.bits(want['totals']))
    assert np.array_equal(x.cpu().numpy(), want['x']) and np.array_equal(viol.cpu().numpy(), want['viol'])
    assert (iters.cpu().numpy() == N_ITER[name]).all()                         # no early stop
    assert torch.equal(dec(cuda(NC.words(name))).detach(), cuda(totals))       # the module's forward is this launch
    # decode mode: the state after the iteration it stops at is the train mode's totals of that iteration
    dx, dviol, diters, dpost = (t.cpu().numpy() for t in dec.decode(cuda(NC.words(name)), want_posteriors=True))
    assert np.array_equal(diters, want['dec_iters']) and np.array_equal(dviol, want['dec_viol']) and np.array_equal(dx, want['dec_x'])
    assert np.array_equal(LG.bits(dpost), LG.bits(totals[diters - 1, np.arange(len(diters))]))
    if name == 'g12':                                                           # a strided llr: llr_sb = N + 5 > N
        wide = torch.full((LG.B, 12 + 5), float('nan'), device='cuda')
        wide[:, :12] = cuda(NC.words(name))
        assert wide[:, :12].stride(0) == 17
        assert torch.equal(train_forward(dec, wide[:, :12])[0], cuda(totals))


def test_the_load_rule_in_both_directions():
    """NaN -> 0 and the clamp to +-4096 in the forward; no gradient through them in the backward."""
    name, share = 'builtin', 'edge'
    alpha, beta = NC.weights(name, share)
    special = NC.words(name)[:8].copy()
    special[0, 3], special[1, 5], special[2, 7] = np.nan, 1e9, -1e9
    dec = module(name, share, alpha, beta)
    want = NO.forward(special, NC.tabs(name), alpha, beta, share, N_ITER[name])
    assert np.array_equal(LG.bits(train_forward(dec, special)[0].cpu().numpy()), LG.bits(want['totals']))
    g = NC.g_totals(name)[:, :8]
    got = device_backward(dec, special, g)
    assert got[2][0, 3] == 0 and got[2][1, 5] == 0 and got[2][2, 7] == 0 and np.count_nonzero(got[2] == 0) == 3
    ref = NO.backward(want, g)                                                  # the f32 recursion: zero at the same places, close elsewhere
    assert np.array_equal(got[2] == 0, ref[2] == 0) and np.allclose(got[2], ref[2], rtol=0, atol=1e-4 * np.abs(ref[2]).max())


@pytest.mark.parametrize('share', SHARES)
@pytest.mark.parametrize('name', CODES)
def test_backward_within_the_restatements_own_error(name, share):
    alpha, beta = NC.weights(name, share)
    keep = NC.kept(name, share)
    assert (~keep).mean() <= NC.LEFT_OUT_CAP
    want = NC.restated_backward(name, share)                                   # float64, on the kept words
    got = device_backward(module(name, share, alpha, beta), NC.words(name)[keep], NC.g_totals(name)[:, keep])
    err = NC.relative_error(got, want)
    own = NC.relative_error(NC.restated_backward(name, share, 'float32'), want)
    print(name, share, 'device error', err, 'restatement f32 error', own, 'bound', list(BOUND.values()), 'words left out', int((~keep).sum()))
    for k, e in zip(BOUND, err):
        assert e <= BOUND[k], (k, e)
    no_llr = device_backward(module(name, share, alpha, beta), NC.words(name)[keep], NC.g_totals(name)[:, keep], want_llr=False)
    assert no_llr[2] is None and np.array_equal(no_llr[0], got[0]) and np.array_equal(no_llr[1], got[1])


@pytest.mark.parametrize('share', SHARES)
def test_backward_is_deterministic_and_loops_over_its_words(share):
    """More words than workgroups: some workgroups take two words.  Two calls return the same bits; the batch's gradient is the sum
    of its halves' within the bound of the comparison with the restatement (another order of the same additions)."""
    from fgnn_amd.ldpc_nms import backward_workgroups
    name = 'g12'
    G = backward_workgroups(10 ** 6)
    assert backward_workgroups(3) == 3 and G >= 64
    sets = -(-(G + 67) // LG.B)
    llr = np.concatenate([received(LG.case(name)[0], 5000 + i, LG.SNR_DB[name], LG.B) for i in range(sets)])
    B = len(llr)
    assert B > G and backward_workgroups(B) == G
    g = np.random.RandomState(4100).standard_normal((N_ITER[name], B, 12)).astype(np.float32)
    dec = module(name, share, *NC.weights(name, share))
    first, again = device_backward(dec, llr, g), device_backward(dec, llr, g)
    for a, b in zip(first, again):
        assert np.array_equal(LG.bits(a), LG.bits(b))
    h = B // 2
    lo, hi = device_backward(dec, llr[:h], g[:, :h]), device_backward(dec, llr[h:], g[:, h:])
    assert np.array_equal(LG.bits(first[2]), LG.bits(np.concatenate([lo[2], hi[2]])))          # a word's g_llr is its own
    for k, full, parts in (('g_alpha', first[0], lo[0].astype(np.float64) + hi[0]), ('g_beta', first[1], lo[1].astype(np.float64) + hi[1])):
        err = float(np.abs(full - parts).max() / np.abs(parts).max())
        print(share, k, 'batch against the sum of its halves', err, 'bound', BOUND[k])
        assert err <= BOUND[k]


def test_module_gradients_are_the_abi_calls():
    from fgnn_amd import _hip
    from fgnn_amd.ldpc_nms import LearnedMinSum, multi_loss, nms_backward_raw, nms_forward_raw
    code = LG.case('builtin')[0]
    dec = LearnedMinSum(code, 5, 'edge').cuda()
    llr = cuda(NC.words('builtin')).requires_grad_()
    cw = torch.from_numpy(np.random.RandomState(7).randint(0, 2, (LG.B, 96)).astype(np.uint8)).cuda()
    totals = dec(llr)
    assert totals.shape == (5, LG.B, 96) and totals.requires_grad
    multi_loss(totals, cw).backward()
    # the same through the raw launches, with the loss's gradient taken by torch
    tables, sizes = (dec.col_ptr, dec.row_ptr, dec.row_edge, dec.row_var), (dec.N, dec.M, dec.E)
    E = dec.E                                                                   # (291: three variables of 96.3.963 have four checks)
    alpha, beta = dec.alpha.detach(), dec.beta.detach()
    raw, record = nms_forward_raw(llr.detach(), tables, sizes, alpha, beta, 5, 2)
    assert torch.equal(raw, totals.detach())
    leaf = raw.clone().requires_grad_()
    multi_loss(leaf, cw).backward()
    g_alpha, g_beta, g_llr = nms_backward_raw(leaf.grad, llr.detach(), tables, sizes, alpha, beta, record, 5, 2)
    assert torch.equal(dec.alpha.grad, g_alpha) and torch.equal(dec.beta.grad, g_beta) and torch.equal(llr.grad, g_llr)
    assert float(g_alpha.abs().max()) > 0 and float(g_beta.abs().max()) > 0 and float(g_llr.abs().max()) > 0
    plain = cuda(NC.words('builtin'))                                           # llr.requires_grad is honoured
    dec.zero_grad()
    multi_loss(dec(plain), cw).backward()
    assert plain.grad is None and torch.equal(dec.alpha.grad, g_alpha)
    with torch.no_grad():
        assert not dec(plain).requires_grad

    # bad arguments through the ABI, real device pointers: the documented codes, and nothing is launched (the outputs keep their fill)
    B, nbytes = LG.B, record.numel()
    out = torch.full((5, B, 96), -7.0, device='cuda')
    rec = torch.full((nbytes,), 255, dtype=torch.uint8, device='cuda')

    def fwd(n=96, it=5, share=2, nb=nbytes):
        return _hip.invoke('fgnn_ldpc_nms_forward', plain, 96, *tables, alpha, beta, B, n, 48, E, it, share, 0, None, None, None, None, out,
                           rec, nb)
    assert fwd(it=0) == -1 and fwd(share=3) == -1 and fwd(nb=nbytes - 1) == -1 and fwd(n=1025) == _hip.EUNSUPPORTED
    ga, gb = torch.full_like(alpha, -7.0), torch.full_like(beta, -7.0)
    ws = torch.empty((int(_hip.invoke('fgnn_ldpc_nms_backward_workspace_bytes', B, 96, 48, E, 5, 2)),), dtype=torch.uint8, device='cuda')

    def bwd(n=96, it=5, share=2, nb=nbytes, wb=ws.numel()):
        return _hip.invoke('fgnn_ldpc_nms_backward', leaf.grad, plain, 96, *tables, alpha, beta, record, nb, B, n, 48, E, it, share, ga, gb,
                           None, ws, wb)
    assert bwd(it=0) == -1 and bwd(share=3) == -1 and bwd(nb=nbytes - 1) == -1 and bwd(wb=ws.numel() - 1) == -1
    assert bwd(n=1025) == _hip.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((rec == 255).all()) and bool((ga == -7.0).all()) and bool((gb == -7.0).all())
    assert bwd() == 0 and torch.equal(ga, g_alpha) and torch.equal(gb, g_beta)


def test_training_lowers_the_loss_and_its_checkpoint_evaluates(paths, tmp_path, monkeypatch):
    """``ldpc_nms_train.train`` on the built-in code: n_iter 5, per-edge weights from alpha = 1, beta = 0, 2 dB, batch 256, 40 steps.

    The same 40 steps through the float64 restatement on the CPU (torch autograd over ``ldpc_nms_oracle.torch_forward``, stock Adam
    at 1e-2, the batches of tests/ldpc_train_oracle.py ``sample_batch(G, 256, 0, step, snr_choices=(2,))``): ``multi_loss`` on the
    held-out batch (step 2^62) 0.317469 before, 0.258550 after; on 8192 further held-out words the decode mode leaves 26828 wrong
    message bits of 393216, min-sum:flooding:iters=5:alpha=1.0 leaves 38812.  So the two assertions below hold for the algorithm."""
    from fgnn_amd import ldpc_eval
    from fgnn_amd.ldpc_nms import LearnedMinSum, load_checkpoint, multi_loss
    from fgnn_amd.ldpc_nms_train import train
    path = paths('builtin')
    runs = {}
    for graph in (True, False):
        runs[graph] = train(n_epochs=1, batch_size=256, snr=2, n_iter=5, share='edge', steps_per_epoch=40, seed=0,
                            out_dir=str(tmp_path / ('graph' if graph else 'eager')), log_every=0, graph=graph, alpha=1.0, beta=0.0)
        assert runs[graph]['steps'] == 40 and runs[graph]['gcnt'] == 40 and len(runs[graph]['losses']) == 40
    assert runs[True]['graphed'] and not runs[False]['graphed']
    assert runs[True]['losses'] == runs[False]['losses']
    ckpt = runs[True]['checkpoint']
    saved = torch.load(ckpt, map_location='cpu', weights_only=True)
    assert set(saved) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt', 'decoder'}      # the default code: no 'code'
    assert saved['decoder'] == {'kind': 'learned-min-sum', 'n_iter': 5, 'share': 'edge'} and (saved['epoch'], saved['gcnt']) == (1, 40)
    trained, fresh = load_checkpoint(ckpt, device='cuda'), LearnedMinSum(None, 5, 'edge', alpha=1.0, beta=0.0).cuda()
    held = path.sample_rng(256, seed=0, step=2 ** 62, snr_db=2)
    llr = path.bit_llr(held.y, held.snr_db)
    with torch.no_grad():
        before, after = float(multi_loss(fresh(llr), held.cw)), float(multi_loss(trained(llr), held.cw))
    print('held-out multi-loss before %.6f after %.6f; first and last training loss %.6f %.6f'
          % (before, after, runs[True]['losses'][0], runs[True]['losses'][-1]))
    assert after < before

    spec, fixed = 'learned-min-sum:' + ckpt, 'min-sum:flooding:iters=5:alpha=1.0'
    ts = path.make_test_set(num=200, snr_db=(2,), baseline=False)               # 1200 words at 2 dB, every burst level
    res = ldpc_eval.evaluate(ZeroLogits().cuda(), ts, baseline=[spec, fixed])
    learned, classical = res['baselines'][spec], res['baselines'][fixed]
    assert learned['counts'].shape == (31, 4) and learned['err_class'].shape == (5, 6)
    assert learned['counts'][-1][0] == 48 * 1200 and learned['counts'][-1][2] == 1200
    print('BER at 2 dB: learned %.5f, %s %.5f' % (learned['ber'], fixed, classical['ber']))
    assert learned['ber'] <= classical['ber']
    single = ldpc_eval.evaluate(ZeroLogits().cuda(), ts, baseline=spec)
    assert np.array_equal(single['baseline']['counts'], learned['counts'])
    rows = ldpc_eval.ber_curve(None, spec, snr_db=(2.0,), batch=256, max_words=512, min_word_errors=10 ** 9)
    assert len(rows) == 1 and rows[0]['words'] == 512 and rows[0]['snr_db'] == 2.0 and 0 < rows[0]['ber'] < 0.5
    assert 1 <= rows[0]['mean_iters'] <= 5
    # two runs of the spec on one path load the checkpoint once, into the dict the path declares
    from fgnn_amd.datapath import LdpcDataPath
    one, loads = LdpcDataPath('cuda:0'), []
    assert one._learned == {}
    monkeypatch.setattr(torch, 'load', lambda f, *a, _load=torch.load, **kw: loads.append(f) or _load(f, *a, **kw))
    decoder = ldpc_eval.parse_decoder(spec)
    first, again = decoder.run(one, held.y, held.snr_db), decoder.run(one, held.y, held.snr_db)
    monkeypatch.undo()
    assert loads == [ckpt] and list(one._learned) == [ckpt] and isinstance(one._learned[ckpt], LearnedMinSum)
    assert len(first) == 3 and all(torch.equal(a, b) for a, b in zip(first, again))
    assert all(torch.equal(a, b) for a, b in zip(first, trained.decode(llr)))
    from fgnn_amd.ldpc_code import LdpcCode
    with pytest.raises(ValueError, match='trained for'):                        # a checkpoint of another code is refused
        ldpc_eval.ber_curve(LdpcCode.gallager(24, 3, 6, 0), spec, snr_db=(2.0,), batch=64, max_words=64)
