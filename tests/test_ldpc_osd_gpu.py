"""GPU: ordered-statistics reprocessing (csrc/ldpc_osd.hip; LdpcDataPath.decode_osd, ldpc_eval's ``osd=`` specs) against the numpy
restatement tests/ldpc_osd_oracle.py.  Every deciding operation is an integer one, so x, cost and pattern are compared bit for bit:
no tolerance and no word left out.

Inputs (``case``): the all-zero codeword sent at one SNR per code (the two large codes: SNRs spread evenly over a range, as in
test_ldpc_llr_gpu.py), 67 words from a fixed numpy seed; ``rel`` is the restatement's layered min-sum posteriors after 20 iterations
(tests/ldpc_llr_oracle.py, bit for bit what the device computes, so nothing here depends on the BP kernel) and ``metric`` the channel
LLRs.  On the 16 x 16 code those posteriors overflow to NaN for the words that do not decode.  The spans: 1, 7, N - rank (every
non-pivot position) and N - rank + 5 (clipped); order 2 stops at 256 positions, and at 32 on the 1024-bit code."""
import functools

import numpy as np
import pytest
import torch

import ldpc_llr_oracle as LO
import ldpc_osd_oracle as OO
from ldpc_decoder_cases import ZeroLogits, code as named_code, make_paths, received

pytestmark = pytest.mark.gpu

B = 67
BP_ITERS = 20
CODES = ('g12', 'g33', 'g63', 'g64', 'builtin', 'g32', 'g384', 'g1024')
SNR_DB = {'g12': (1.0, 1.0), 'g33': (3.0, 3.0), 'g63': (3.0, 3.0), 'g64': (3.0, 3.0), 'builtin': (2.5, 2.5), 'g32': (3.0, 3.0),
          'g384': (0.5, 6.5), 'g1024': (1.0, 7.0)}          # (lo, hi) dB


@functools.lru_cache(maxsize=None)
def case(name):
    """(code, tables, H [M, N], llr [B, N] f32, the min-sum restatement's result on llr) of one code: computed once, never written."""
    code = named_code(name)                 # (ldpc_decoder_cases.CODES says why each is here)
    tabs = LO.tables(code.nlist, code.n_chk)
    H = OO.dense(tabs[1], tabs[3], code.n_var)
    llr = received(code, 3000 + CODES.index(name), SNR_DB[name], B)
    bp = LO.decode(llr, tabs, code.layers(), 'min-sum', BP_ITERS)
    bp['post'].setflags(write=False)
    return code, tabs, H, llr, bp


@functools.lru_cache(maxsize=None)
def eliminated(name):
    """The restatement's per-word states for ``case(name)`` with every word reprocessed; shared among (order, span)."""
    _, _, H, llr, bp = case(name)
    return OO.states(bp['post'], llr, H)


def free_positions(name):
    return len(eliminated(name)[0]['free'])                 # N - rank


def settings(name):
    """The (order, span) pairs of one code."""
    nf = free_positions(name)
    cap = 32 if name == 'g1024' else 256
    return ([(0, 1), (0, nf + 5)] + [(1, s) for s in (1, 7, nf, nf + 5)]
            + [(2, s) for s in sorted({1, 7, min(nf, cap), min(nf + 5, cap)})])


@functools.lru_cache(maxsize=None)
def restated(name, order, span):
    _, _, H, llr, bp = case(name)
    return OO.reprocess(bp['post'], llr, None, H, order, span, eliminated(name))


paths = pytest.fixture(scope='module', name='paths')(make_paths)


def dev(a, dtype=np.float32):
    return None if a is None else a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype)).cuda()


def run(path, rel, metric=None, viol=None, **kw):
    x, cost, pattern = path.decode_osd(dev(rel), dev(metric), dev(viol, np.int32), **kw)
    assert x.dtype == torch.uint8 and cost.dtype == torch.int32 and pattern.dtype == torch.int32
    return x.cpu().numpy(), cost.cpu().numpy(), pattern.cpu().numpy()


def assert_same(got, want, rows=slice(None)):
    for g, w, what in zip(got, want, ('x', 'cost', 'pattern')):
        assert np.array_equal(g, w[rows]), what


@pytest.mark.parametrize('name', CODES)
def test_equals_the_restatement_bit_for_bit(paths, name):
    code, _, H, llr, bp = case(name)
    assert free_positions(name) == code.n_var - int(len(eliminated(name)[0]['piv']))
    assert (bp['viol'] != 0).any()
    winners = set()
    for order, span in settings(name):
        want = restated(name, order, span)
        got = run(paths(name), bp['post'], llr, order=order, span=span)
        assert_same(got, want)
        assert not (H.astype(np.int64) @ got[0].T.astype(np.int64) % 2).any()          # every output satisfies every check
        winners |= set(want[2].tolist())
    assert len(winners) > 1 and 0 in winners                                           # (the inputs make more than one candidate win)
    order, span = settings(name)[-1]
    assert_same(run(paths(name), bp['post'][:1], llr[:1], order=order, span=span), restated(name, order, span), slice(0, 1))   # B = 1


@pytest.mark.parametrize('name', ('g12', 'builtin', 'g32', 'g384'))
def test_ties_and_specials(paths, name):
    code, _, H, llr, bp = case(name)
    N, path = code.n_var, paths(name)
    rng = np.random.RandomState(7)
    tied = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0], np.float32), (9, N))             # four reliabilities only: ties by index
    zeros = np.zeros((3, N), np.float32)
    zeros[1] = -0.0
    special = np.array(llr[:9])
    special[0, 3 % N], special[1, 5 % N], special[2, 7 % N] = np.nan, np.inf, -np.inf
    special[3, :] = np.nan
    special[4, ::2], special[5, 1::3], special[6, :] = np.inf, -np.inf, 1e9
    special[7, 0], special[8, N - 1] = 1e-9, -4096.5
    for rel, metric in ((tied, tied), (tied, llr[:9]), (zeros, zeros), (zeros, llr[:3]), (special, llr[:9]), (llr[:9], special),
                        (special, special)):
        for order, span in ((0, 1), (1, N), (2, 9)):
            want = OO.reprocess(rel, metric, None, H, order, span)
            assert_same(run(path, rel, metric, order=order, span=span), want)
    want = OO.reprocess(zeros, zeros, None, H, 1, N)
    assert not want[0].any() and not want[1].any() and not want[2].any()                # all zeros: the all-zero word at no cost


def test_metric_none_strides_and_defaults(paths):
    code, _, H, llr, bp = case('builtin')
    path, N = paths('builtin'), 96
    want = OO.reprocess(bp['post'], None, None, H, 1, N)
    assert_same(run(path, bp['post'], None, order=1, span=N), want)                      # metric=None is metric=rel
    assert_same(run(path, bp['post'], bp['post'], order=1, span=N), want)
    wide = torch.full((B, 2 * N + 5), float('nan'), device='cuda')                       # strided rows: rel_sb = metric_sb = 2 N + 5
    wide[:, :N] = dev(bp['post'])
    wide[:, N + 5:] = dev(llr)
    rel, metric = wide[:, :N], wide[:, N + 5:]
    assert rel.stride(0) == 2 * N + 5 == metric.stride(0) and metric.data_ptr() != rel.data_ptr()
    assert_same(run(path, rel, metric, order=2, span=24), OO.reprocess(bp['post'], llr, None, H, 2, 24, eliminated('builtin')))
    assert_same(run(path, bp['post'], llr), OO.reprocess(bp['post'], llr, None, H, 1, N, eliminated('builtin')))           # order 1, span N
    assert_same(run(path, bp['post'], llr, order=2), OO.reprocess(bp['post'], llr, None, H, 2, 64, eliminated('builtin')))  # span 64
    assert_same(run(path, bp['post'].astype(np.float64), torch.from_numpy(np.array(llr)).double(), order=0),                # f64 in
                restated('builtin', 0, 1))
    x, cost, pattern = path.decode_osd(torch.zeros(0, N, device='cuda'))                 # B = 0: no launch
    assert x.shape == (0, N) and cost.shape == (0,) and pattern.shape == (0,)


@pytest.mark.parametrize('name', ('builtin', 'g32', 'g1024'))
def test_pass_through_words(paths, name):
    code, _, H, llr, bp = case(name)
    viol = bp['viol'].astype(np.int32)
    assert (viol == 0).any() and (viol != 0).any()
    for mask in (viol, np.where(np.arange(B) % 3 == 0, 0, 1).astype(np.int32)):         # the decoder's own, and an arbitrary one
        want = OO.reprocess(bp['post'], llr, mask, H, 1, 7)
        got = run(paths(name), bp['post'], llr, mask, order=1, span=7)
        assert_same(got, want)
        through = mask == 0
        with np.errstate(invalid='ignore'):
            h = (bp['post'] < 0).astype(np.uint8)
        assert (got[2][through] == -1).all() and (got[2][~through] >= 0).all() and np.array_equal(got[0][through], h[through])
        c0 = (OO.quantise(llr) * (h ^ (llr < 0))).sum(1)
        assert np.array_equal(got[1][through], c0[through])
        full = restated(name, 1, 7)                                                      # the other words: as without a mask
        assert all(np.array_equal(g[~through], f[~through]) for g, f in zip(got, full))


def raw(row_ptr, row_var, N, rel, metric, order, span):
    """Through the C ABI with hand-built CSR tables."""
    from fgnn_amd import _hip
    M, E, nb = len(row_ptr) - 1, len(row_var), rel.shape[0]
    rp, rv = dev(row_ptr, np.int32), dev(row_var, np.int32)
    r, m = dev(rel), dev(metric)
    x = torch.full((nb, N), 9, device='cuda', dtype=torch.uint8)
    cost, pattern = (torch.full((nb,), -7, device='cuda', dtype=torch.int32) for _ in range(2))
    _hip.call('fgnn_ldpc_osd', r, N, m, N, None, rp, rv, nb, N, M, E, order, span, x, cost, pattern)
    assert _hip.lib().fgnn_last_kernel().decode().startswith('ldpc_osd_kernel')
    return x.cpu().numpy(), cost.cpu().numpy(), pattern.cpu().numpy()


def test_raw_abi_irregular_and_tall():
    rng = np.random.RandomState(11)
    # irregular: N = 40, M = 13, row weights 1..9, two equal rows and a variable in no check
    N, M = 40, 13
    rows = [sorted(rng.choice(N - 1, 1 + (m * 5) % 9, replace=False).tolist()) for m in range(M)]
    rows[7] = list(rows[2])
    # tall: N = 20, M = 70 > N (two rows per thread); row weights 2 and 4 over 18 of the variables, so the rank is at most 17
    tall = [sorted(rng.choice(18, 2 + 2 * (m % 2), replace=False).tolist()) for m in range(70)]
    for n_var, rws in ((N, rows), (20, tall)):
        row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rws])]).astype(np.int32)
        row_var = np.array([v for r in rws for v in r], np.int32)
        H = OO.dense(row_ptr, row_var, n_var)
        rel = (rng.standard_normal((B, n_var)) * 2).astype(np.float32)
        metric = (rel + rng.standard_normal((B, n_var))).astype(np.float32)
        nf = n_var - len(OO.eliminate(rel[0], metric[0], H)['piv'])
        assert nf >= 1
        for order, span in ((0, 1), (1, 1), (1, nf), (1, nf + 3), (2, 2), (2, nf + 3)):
            want = OO.reprocess(rel, metric, None, H, order, span)
            got = raw(row_ptr, row_var, n_var, rel, metric, order, span)
            assert_same(got, want)
            assert not (H.astype(np.int64) @ got[0].T.astype(np.int64) % 2).any()


def test_run_decoder_is_the_composition(paths):
    from fgnn_amd import ldpc_eval
    code, tabs, H, llr, bp = case('builtin')
    path = paths('builtin')
    snr = np.full(B, SNR_DB['builtin'][0], np.float32)
    gcx = np.float32(10.0) ** (snr / np.float32(20.0))
    y = torch.from_numpy(np.array(llr) / (-2.0 * gcx[:, None])).cuda()
    dllr = path.bit_llr(y, torch.from_numpy(snr).cuda()).cpu().numpy()                   # what Decoder.run feeds the decoder
    for spec, order, span in (('min-sum:layered:iters=20:osd=1', 1, 96), ('min-sum:layered:iters=20:osd=2:span=24', 2, 24),
                              ('min-sum:layered:iters=20:osd=0', 0, 96)):
        x, viol, iters = ldpc_eval.parse_decoder(spec).run(path, y, torch.from_numpy(snr).cuda())
        wx, _, _, r = OO.bp_osd(dllr, tabs, code.layers(), H, order, span, 'min-sum', BP_ITERS)
        assert np.array_equal(x.cpu().numpy(), wx) and not viol.any().item() and np.array_equal(iters.cpu().numpy(), r['iters'])
        assert not (H.astype(np.int64) @ wx.T.astype(np.int64) % 2).any()


def test_evaluate_and_ber_curve_count_what_the_restatement_counts(paths):
    from fgnn_amd import ldpc_eval
    from fgnn_amd.datapath import LdpcDataPath
    code, tabs, H, _, _ = case('builtin')
    path = paths('builtin')
    spec = 'min-sum:layered:iters=20:osd=1'
    ts = path.make_test_set(num=2, baseline=False)
    res = ldpc_eval.evaluate(ZeroLogits().cuda(), ts, baseline=[spec, 'min-sum:layered:iters=20'])
    y, gts, snr = ts['noizy_sg'].numpy(), ts['gts'].numpy(), ts['snr_dbs'].numpy()[:, 0]
    llr = path.bit_llr(ts['noizy_sg'], ts['snr_dbs'][:, 0]).cpu().numpy()
    wx = OO.bp_osd(llr, tabs, code.layers(), H, 1, 96, 'min-sum', BP_ITERS)[0]
    wrong = wx[:, :48] != gts[:, :48]
    assert list(res['baselines'][spec]['counts'][-1]) == [48 * len(y), int(wrong.sum()), len(y), int(wrong.any(1).sum())]

    rows = ldpc_eval.ber_curve(code, spec, [2.5], batch=64, max_words=128, min_word_errors=10 ** 9)
    assert len(rows) == 1 and rows[0]['words'] == 128
    curve = LdpcDataPath('cuda:0', code)
    curve.sigma_b_choices = (0,)
    bit_errors = word_errors = 0
    for j in range(2):
        drawn = curve.sample_rng(64, seed=0, step=j, snr_db=2.5)
        wx = OO.bp_osd(curve.bit_llr(drawn.y, drawn.snr_db).cpu().numpy(), tabs, code.layers(), H, 1, 96, 'min-sum', BP_ITERS)[0]
        wrong = wx[:, :48] != drawn.cw.cpu().numpy()[:, :48]
        bit_errors, word_errors = bit_errors + int(wrong.sum()), word_errors + int(wrong.any(1).sum())
    assert (rows[0]['bit_errors'], rows[0]['word_errors']) == (bit_errors, word_errors)
