"""GPU: the layered learned min-sum LDPC decoder (csrc/ldpc_nms_layered.hip; fgnn_amd/ldpc_nms.py's ``schedule='layered'``,
ldpc_nms_train's ``schedule``, ldpc_eval's learned-min-sum spec) against the existing LLR-domain kernel's layered schedule and the
restatement tests/ldpc_nms_layered_oracle.py.

Inputs are tests/test_ldpc_nms_layered.py's (``code``, ``words``, ``weights``, ``g_totals``), and so are the yardstick and its
measurement: ``D``, per output tensor the largest |g_f32 - g_f64| / max |g_f64| between the restatement's own two precisions,
g_alpha 6.890e-07, g_beta 3.033e-07, g_llr 2.656e-07, measured on the CPU by ``test_ldpc_nms_layered.restatement_error`` over every
(code, share) of its BACKWARD_CODES.  The backward's bound is 4 d per tensor: the device adds the words and the edges in another
order than numpy does, errors of the size that separate the two precisions.  Only words whose f32 and f64 records agree in every
field are given to the device (``kept``; on these inputs that is every word, asserted on the CPU).

Forward: every operation is an IEEE f32 add, subtract, multiply, maximum or compare in a fixed order, so the decode mode with
constant weights equals fgnn_ldpc_decode_llr's layered min-sum / offset min-sum bit for bit, and the train mode's totals equal the
f32 restatement bit for bit."""
import numpy as np
import pytest
import torch

import ldpc_nms_layered_oracle as YO
from ldpc_decoder_cases import ZeroLogits, received
import test_ldpc_llr_gpu as LG
import test_ldpc_nms_layered as LC

pytestmark = pytest.mark.gpu

SHARES, N_ITER = LC.SHARES, LC.N_ITER
BOUND = {k: 4 * d for k, d in LC.D.items()}


@pytest.fixture(scope='module')
def paths():
    from fgnn_amd.datapath import LdpcDataPath
    made = {}

    def get(name):
        if name not in made:
            made[name] = LdpcDataPath('cuda:0', LC.code(name))
        return made[name]
    return get


def cuda(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()       # (a copy in C order: a[:, mask] comes with strides of its own)


def module(name, share, alpha, beta):
    """A layered ``LearnedMinSum`` on the device holding the given weights ([n_iter, W] arrays)."""
    from fgnn_amd.ldpc_nms import LearnedMinSum
    dec = LearnedMinSum(LC.code(name), alpha.shape[0], share, schedule='layered').cuda()
    with torch.no_grad():
        dec.alpha.copy_(cuda(alpha))
        dec.beta.copy_(cuda(beta))
    return dec


class Raw:
    """The arguments of the raw launches for tables built by hand (``module``'s attributes without an ``LdpcCode``)."""

    def __init__(self, tabs, layers, alpha, beta, share):
        self.col_ptr, self.row_ptr, self.row_edge, self.row_var = (cuda(np.asarray(a, np.int32)) for a in tabs)
        self.layer_ptr, self.layer_chk = (cuda(np.asarray(a, np.int32)) for a in layers)
        self.N, self.M, self.E = len(tabs[0]) - 1, len(tabs[1]) - 1, len(tabs[2])
        self.alpha, self.beta, self.n_iter, self.share = cuda(alpha), cuda(beta), alpha.shape[0], share


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
    _hip.call('fgnn_ldpc_nms_layered_forward', llr, llr.stride(0), dec.col_ptr, dec.row_ptr, dec.row_edge, dec.row_var, dec.layer_ptr,
              dec.layer_chk, dec.layer_ptr.numel() - 1, dec.alpha.detach(), dec.beta.detach(), B, N, M, E, dec.n_iter,
              SHARES.index(dec.share), 0, x, None, viol, iters, totals, record, nbytes)
    return totals, record, x, viol, iters


def device_backward(dec, llr, g, want_llr=True):
    """Forward (train mode) and backward through the raw launches: (g_alpha, g_beta, g_llr) as numpy arrays."""
    from fgnn_amd.ldpc_nms import nms_backward_raw, nms_forward_raw
    llr, g = cuda(llr), cuda(g)
    tables, sizes, share = (dec.col_ptr, dec.row_ptr, dec.row_edge, dec.row_var), (dec.N, dec.M, dec.E), SHARES.index(dec.share)
    layers = (dec.layer_ptr, dec.layer_chk)
    alpha, beta = dec.alpha.detach(), dec.beta.detach()
    _, record = nms_forward_raw(llr, tables, sizes, alpha, beta, dec.n_iter, share, layers)
    out = nms_backward_raw(g, llr, tables, sizes, alpha, beta, record, dec.n_iter, share, want_llr, layers)
    return tuple(None if t is None else t.cpu().numpy() for t in out)


@pytest.mark.parametrize('name', LC.FORWARD_CODES)
def test_decode_mode_with_constant_weights_is_the_layered_llr_kernel_bit_for_bit(paths, name):
    llr = cuda(LG.case(name)[3] if name != 'w1024' else received(LC.code(name), 1237, (3.0, 3.0), LG.B))
    it = LG.MS_ITERS
    for algorithm, alpha, beta in (('min-sum', 0.8125, 0.0), ('offset-min-sum', 1.0, 0.5)):
        dec = module(name, 'iteration', np.full((it, 1), alpha, np.float32), np.full((it, 1), beta, np.float32))
        for rows in (slice(None), slice(0, 1)):                                # B = 67, B = 1
            want = paths(name).decode_llr(llr[rows], algorithm, 'layered', max_iter=it, alpha=0.8125, beta=0.5, want_posteriors=True)
            got = dec.decode(llr[rows], want_posteriors=True)
            for g, w in zip(got[:3], want[:3]):
                assert g.dtype == w.dtype and torch.equal(g, w)
            post, ref = got[3].cpu().numpy(), want[3].cpu().numpy()
            nan = np.isnan(ref)                                                 # NaN places are compared as places
            assert np.array_equal(np.isnan(post), nan) and np.array_equal(LG.bits(post)[~nan], LG.bits(ref)[~nan])
        assert dec.decode(llr)[0].shape == llr.shape and len(dec.decode(llr)) == 3
        assert dec.decode(torch.zeros(0, llr.shape[1], device='cuda'))[0].shape == (0, llr.shape[1])       # B = 0: no launch


@pytest.mark.parametrize('share', SHARES)
@pytest.mark.parametrize('name', LC.FORWARD_CODES)
def test_train_mode_equals_the_restatement_bit_for_bit(name, share):
    alpha, beta = LC.weights(name, share)
    want = LC.restated(name, share)
    dec = module(name, share, alpha, beta)
    totals, _, x, viol, iters = train_forward(dec, LC.words(name))
    totals = totals.cpu().numpy()
    nan = np.isnan(want['totals'])                                              # (g32: none on these inputs, asserted)
    assert not nan.any() and np.array_equal(LG.bits(totals), LG.bits(want['totals']))
    assert np.array_equal(x.cpu().numpy(), want['x']) and np.array_equal(viol.cpu().numpy(), want['viol'])
    assert (iters.cpu().numpy() == N_ITER[name]).all()                         # no early stop
    assert torch.equal(dec(cuda(LC.words(name))).detach(), cuda(totals))       # the module's forward is this launch
    # decode mode: the state after the iteration it stops at is the train mode's totals of that iteration
    dx, dviol, diters, dpost = (t.cpu().numpy() for t in dec.decode(cuda(LC.words(name)), want_posteriors=True))
    assert np.array_equal(diters, want['dec_iters']) and np.array_equal(dviol, want['dec_viol']) and np.array_equal(dx, want['dec_x'])
    assert np.array_equal(LG.bits(dpost), LG.bits(totals[diters - 1, np.arange(len(diters))]))
    if name == 'g12':                                                           # a strided llr: llr_sb = N + 5 > N
        wide = torch.full((LG.B, 12 + 5), float('nan'), device='cuda')
        wide[:, :12] = cuda(LC.words(name))
        assert wide[:, :12].stride(0) == 17
        assert torch.equal(train_forward(dec, wide[:, :12])[0], cuda(totals))


@pytest.mark.parametrize('share', SHARES)
def test_an_irregular_matrix_with_a_degree_one_check_through_the_raw_abi(share):
    """The only place L = 1 meets L > 1; the layer order is not index order.  Forward bits, and the backward against the float64
    restatement within the bound on the words whose records agree."""
    name = 'irregular'
    alpha, beta = LC.weights(name, share)
    raw = Raw(LC.tabs(name), LC.layers(name), alpha, beta, share)
    want = LC.restated(name, share)
    totals, _, x, viol, iters = train_forward(raw, LC.words(name))
    assert np.array_equal(LG.bits(totals.cpu().numpy()), LG.bits(want['totals']))
    assert np.array_equal(x.cpu().numpy(), want['x']) and np.array_equal(viol.cpu().numpy(), want['viol'])
    assert (iters.cpu().numpy() == N_ITER[name]).all()
    keep = LC.kept(name, share)
    assert (~keep).mean() <= LC.LEFT_OUT_CAP
    got = device_backward(raw, LC.words(name)[keep], LC.g_totals(name)[:, keep])
    ref = LC.restated_backward(name, share)
    err = LC.relative_error(got, ref)
    print(share, 'device error', err, 'bound', list(BOUND.values()), 'words left out', int((~keep).sum()))
    for k, e in zip(BOUND, err):
        assert e <= BOUND[k], (k, e)


def test_the_load_rule_in_both_directions():
    """NaN -> 0 and the clamp to +-4096 in the forward; no gradient through them in the backward."""
    name, share = 'builtin', 'edge'
    alpha, beta = LC.weights(name, share)
    special = LC.words(name)[:8].copy()
    special[0, 3], special[1, 5], special[2, 7] = np.nan, 1e9, -1e9
    dec = module(name, share, alpha, beta)
    want = YO.forward(special, LC.tabs(name), LC.layers(name), alpha, beta, share, N_ITER[name])
    assert np.array_equal(LG.bits(train_forward(dec, special)[0].cpu().numpy()), LG.bits(want['totals']))
    g = LC.g_totals(name)[:, :8]
    got = device_backward(dec, special, g)
    assert got[2][0, 3] == 0 and got[2][1, 5] == 0 and got[2][2, 7] == 0 and np.count_nonzero(got[2] == 0) == 3
    ref = YO.backward(want, g)                                                  # the f32 recursion: zero at the same places, close elsewhere
    assert np.array_equal(got[2] == 0, ref[2] == 0) and np.allclose(got[2], ref[2], rtol=0, atol=1e-4 * np.abs(ref[2]).max())


@pytest.mark.parametrize('share', SHARES)
@pytest.mark.parametrize('name', LC.BACKWARD_CODES)
def test_backward_within_the_restatements_own_error(name, share):
    alpha, beta = LC.weights(name, share)
    keep = LC.kept(name, share)
    assert (~keep).mean() <= LC.LEFT_OUT_CAP
    want = LC.restated_backward(name, share)                                   # float64, on the kept words
    got = device_backward(module(name, share, alpha, beta), LC.words(name)[keep], LC.g_totals(name)[:, keep])
    err = LC.relative_error(got, want)
    own = LC.relative_error(LC.restated_backward(name, share, 'float32'), want)
    print(name, share, 'device error', err, 'restatement f32 error', own, 'bound', list(BOUND.values()), 'words left out', int((~keep).sum()))
    for k, e in zip(BOUND, err):
        assert e <= BOUND[k], (k, e)
    no_llr = device_backward(module(name, share, alpha, beta), LC.words(name)[keep], LC.g_totals(name)[:, keep], want_llr=False)
    assert no_llr[2] is None and np.array_equal(no_llr[0], got[0]) and np.array_equal(no_llr[1], got[1])


@pytest.mark.parametrize('share', SHARES)
def test_backward_is_deterministic_and_loops_over_its_words(share):
    """More words than workgroups: some workgroups take two words.  Two calls return the same bits; the batch's gradient is the sum
    of its halves' within the bound of the comparison with the restatement (another order of the same additions)."""
    from fgnn_amd.ldpc_nms import backward_workgroups
    name = 'g12'
    G = backward_workgroups(10 ** 6)
    sets = -(-(G + 67) // LG.B)
    llr = np.concatenate([received(LC.code(name), 5100 + i, LG.SNR_DB[name], LG.B) for i in range(sets)])
    B = len(llr)
    assert B > G == 512 and backward_workgroups(B) == G
    g = np.random.RandomState(4300).standard_normal((N_ITER[name], B, 12)).astype(np.float32)
    dec = module(name, share, *LC.weights(name, share))
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


def test_module_gradients_are_the_layered_abi_calls():
    from fgnn_amd.ldpc_nms import LearnedMinSum, multi_loss, nms_backward_raw, nms_forward_raw
    dec = LearnedMinSum(LC.code('builtin'), 5, 'edge', schedule='layered').cuda()
    llr = cuda(LC.words('builtin')).requires_grad_()
    cw = torch.from_numpy(np.random.RandomState(7).randint(0, 2, (LG.B, 96)).astype(np.uint8)).cuda()
    totals = dec(llr)
    assert totals.shape == (5, LG.B, 96) and totals.requires_grad
    multi_loss(totals, cw).backward()
    tables, sizes, layers = (dec.col_ptr, dec.row_ptr, dec.row_edge, dec.row_var), (dec.N, dec.M, dec.E), (dec.layer_ptr, dec.layer_chk)
    alpha, beta = dec.alpha.detach(), dec.beta.detach()
    raw, record = nms_forward_raw(llr.detach(), tables, sizes, alpha, beta, 5, 2, layers)
    assert torch.equal(raw, totals.detach())
    assert not torch.equal(raw, nms_forward_raw(llr.detach(), tables, sizes, alpha, beta, 5, 2)[0])      # not the flooding launch
    leaf = raw.clone().requires_grad_()
    multi_loss(leaf, cw).backward()
    g_alpha, g_beta, g_llr = nms_backward_raw(leaf.grad, llr.detach(), tables, sizes, alpha, beta, record, 5, 2, layers=layers)
    assert torch.equal(dec.alpha.grad, g_alpha) and torch.equal(dec.beta.grad, g_beta) and torch.equal(llr.grad, g_llr)
    assert float(g_alpha.abs().max()) > 0 and float(g_beta.abs().max()) > 0 and float(g_llr.abs().max()) > 0


def test_training_lowers_the_loss_and_its_checkpoint_evaluates(paths, tmp_path):
    """``ldpc_nms_train.train(schedule='layered')`` on the built-in code: n_iter 5, per-edge weights from alpha = 1, beta = 0, 2 dB,
    batch 256, 40 steps, as tests/test_ldpc_nms_gpu.py trains the flooding decoder.  No BER ranking against flooding is asserted
    (nobody has measured one): the figures are printed."""
    from fgnn_amd import ldpc_eval
    from fgnn_amd.ldpc_nms import LearnedMinSum, load_checkpoint, multi_loss
    from fgnn_amd.ldpc_nms_train import train
    path = paths('builtin')
    runs = {}
    for graph in (True, False):
        runs[graph] = train(n_epochs=1, batch_size=256, snr=2, n_iter=5, share='edge', steps_per_epoch=40, seed=0, schedule='layered',
                            out_dir=str(tmp_path / ('graph' if graph else 'eager')), log_every=0, graph=graph, alpha=1.0, beta=0.0)
        assert runs[graph]['steps'] == 40 and runs[graph]['gcnt'] == 40 and len(runs[graph]['losses']) == 40
    assert runs[True]['graphed'] and not runs[False]['graphed']
    assert runs[True]['losses'] == runs[False]['losses']
    ckpt = runs[True]['checkpoint']
    assert 'LearnedMinSum_edge_layered_5_epoches_1_snr_2.pt' in ckpt
    saved = torch.load(ckpt, map_location='cpu', weights_only=True)
    assert saved['decoder'] == {'kind': 'learned-min-sum', 'n_iter': 5, 'share': 'edge', 'schedule': 'layered'}
    assert (saved['epoch'], saved['gcnt']) == (1, 40)
    trained, fresh = load_checkpoint(ckpt, device='cuda'), LearnedMinSum(None, 5, 'edge', alpha=1.0, beta=0.0, schedule='layered').cuda()
    assert trained.schedule == 'layered'
    held = path.sample_rng(256, seed=0, step=2 ** 62, snr_db=2)
    llr = path.bit_llr(held.y, held.snr_db)
    with torch.no_grad():
        before, after = float(multi_loss(fresh(llr), held.cw)), float(multi_loss(trained(llr), held.cw))
    print('held-out multi-loss before %.6f after %.6f; first and last training loss %.6f %.6f'
          % (before, after, runs[True]['losses'][0], runs[True]['losses'][-1]))
    assert after < before

    flooding = train(n_epochs=1, batch_size=256, snr=2, n_iter=5, share='edge', steps_per_epoch=40, seed=0, out_dir=str(tmp_path / 'flooding'),
                     log_every=0, alpha=1.0, beta=0.0)['checkpoint']
    spec, other, fixed = 'learned-min-sum:' + ckpt, 'learned-min-sum:' + flooding, 'min-sum:layered:iters=5:alpha=1.0'
    ts = path.make_test_set(num=200, snr_db=(2,), baseline=False)               # 1200 words at 2 dB, every burst level
    res = ldpc_eval.evaluate(ZeroLogits().cuda(), ts, baseline=[spec, other, fixed])
    learned = res['baselines'][spec]
    assert learned['counts'].shape == (31, 4) and learned['counts'][-1][0] == 48 * 1200 and learned['counts'][-1][2] == 1200
    print('BER at 2 dB, 5 iterations: trained layered %.5f, trained flooding %.5f, %s %.5f'
          % (learned['ber'], res['baselines'][other]['ber'], fixed, res['baselines'][fixed]['ber']))
    assert 0 < learned['ber'] < 0.5
    decoder = ldpc_eval.parse_decoder(spec)                                     # the spec runs the checkpoint's schedule
    got = decoder.run(path, held.y, held.snr_db)
    assert path._learned[ckpt].schedule == 'layered' and load_checkpoint(flooding).schedule == 'flooding'
    assert all(torch.equal(a, b) for a, b in zip(got, trained.decode(llr)))
