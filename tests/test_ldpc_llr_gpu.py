"""GPU: the LLR-domain LDPC decoders (csrc/ldpc_llr.hip; LdpcDataPath.decode_llr, ldpc_eval.evaluate / ber_curve) against the numpy
restatement tests/ldpc_llr_oracle.py.

Inputs: the all-zero codeword sent at one SNR per code (``SNR_DB``), y = -gcx + z with z from a fixed numpy seed, llr = -2 gcx y in
f32.  The two large codes have no single SNR at which 67 words hold all three kinds the inputs must hold (a word of 384 or 1024 bits
is clean after one iteration only from about 5 dB on, where every word decodes), so their words are sent at SNRs spread evenly over
a range, word b at lo + (hi - lo) b / 66.  The LLRs are of order 1 and every message is a sum, difference, minimum or small multiple
of such values (or an exact zero), far above the f32 denormal range (1.2e-38), so flushing of denormals cannot enter the bit-for-bit
comparison.

Min-sum and offset min-sum: every operation is an IEEE f32 add, subtract, multiply, minimum or compare in a fixed order, so x, viol,
iters and post equal the float32 restatement bit for bit.  On the 16 x 16 code the layered min-sum totals of words that do not decode
grow past the f32 range within the 20 iterations; infinities are compared like any value, and a NaN (inf - inf) must stand at the
same place in both, its sign and payload aside.

Sum-product: the device's tanhf / atanhf are not numpy's.  The yardstick is the float64 restatement; d, the largest
|post_f32 - post_f64| / max(1, |post_f64|) between the restatement's own two precisions over the sum-product inputs (five codes,
both schedules, max_iter 1, 3 and 8; measured on the CPU by ``restatement_error``), is 5.066e-06 and the bound is 4 d = 2.0264e-05
(``SP_BOUND``): device transcendentals differ from numpy's by a few ulp per call, errors of the size that separate the two
precisions, and pass through the same recursion.  x, viol and iters must equal the yardstick's on every word whose margin (smallest
|T| over its run) exceeds the bound; at most 5 % of the words may be left out (asserted; the most in any case is 2 of 67).
The sum-product inputs are sent at lower SNRs (``SP_SNR_DB``) than the min-sum ones: in f32 a tanh rounds to 1 once a message passes
about 17, after which the two precisions of the restatement differ by whole messages (d of 0.01 to 1 from 2 dB on), and the lowest
margin of a 1024-bit word is near 1e-4, so only where d stays near 1e-6 does the comparison hold the 5 % cap."""
import functools

import numpy as np
import pytest
import torch

import ldpc_llr_oracle as LO
from ldpc_decoder_cases import ZeroLogits, code as named_code, make_paths, received

pytestmark = pytest.mark.gpu

B = 67                       # not a multiple of any words-per-workgroup choice
MS_ITERS = 20
SP_ITERS = (1, 3, 8)
SP_D = 5.066e-06             # measured: restatement_error() (module docstring)
SP_BOUND = 4 * SP_D
SCHEDULES = ('flooding', 'layered')
CODES = ('g12', 'builtin', 'g32', 'g384', 'g1024')
# the SNR (or, for the two large codes, the SNR range) per code at which, of the 67 words, some decode, some do not and at least one
# is clean after the first iteration
# (min-sum, flooding, MS_ITERS iterations; asserted in test_inputs_hold_all_three_kinds)
SP_SNR_DB = {'g12': (0.0, 0.0), 'builtin': (0.0, 0.0), 'g32': (0.0, 0.0), 'g384': (0.0, 0.0), 'g1024': (1.0, 1.0)}
SNR_DB = {'g12': (3.0, 3.0), 'builtin': (2.5, 2.5), 'g32': (3.0, 3.0), 'g384': (0.5, 6.5), 'g1024': (1.0, 7.0)}      # (lo, hi) dB


@functools.lru_cache(maxsize=None)
def case(name, sum_product=False):
    """(code, tables, layers, llr [B, N] f32) of one code: the min-sum inputs, or the sum-product ones."""
    if sum_product:
        code, tabs, layers, _ = case(name)
        return code, tabs, layers, received(code, 2000 + CODES.index(name), SP_SNR_DB[name], B)
    code = named_code(name)                 # (ldpc_decoder_cases.CODES says why each is here)
    return code, LO.tables(code.nlist, code.n_chk), code.layers(), received(code, 1000 + CODES.index(name), SNR_DB[name], B)


@functools.lru_cache(maxsize=None)
def restated(name, algorithm, schedule, max_iter, dtype='float32'):
    """The restatement on ``case(name)``'s words: computed once, shared, never written."""
    code, tabs, layers, llr = case(name, algorithm == 'sum-product')
    return LO.decode(llr, tabs, layers if schedule == 'layered' else None, algorithm, max_iter, dtype=np.dtype(dtype))


def restatement_error():
    """(d, the largest number of words within 4 d of a decision boundary in any case) over the sum-product cases; run on the CPU."""
    d, cases = 0.0, []
    for name in CODES:
        for schedule in SCHEDULES:
            for it in SP_ITERS:
                a, b = restated(name, 'sum-product', schedule, it), restated(name, 'sum-product', schedule, it, 'float64')
                d = max(d, float((np.abs(a['post'].astype(np.float64) - b['post']) / np.maximum(1.0, np.abs(b['post']))).max()))
                cases.append(b['margin'])
    return d, max(int((m <= 4 * d).sum()) for m in cases)


paths = pytest.fixture(scope='module', name='paths')(make_paths)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(path, llr, **kw):
    if not isinstance(llr, torch.Tensor):
        llr = torch.from_numpy(np.array(llr, np.float32)).cuda()
    x, viol, iters, post = path.decode_llr(llr, want_posteriors=True, **kw)
    return x.cpu().numpy(), viol.cpu().numpy(), iters.cpu().numpy(), post.cpu().numpy()


def assert_bitwise(got, want, rows=slice(None)):
    x, viol, iters, post = got
    assert np.array_equal(x, want['x'][rows])
    assert np.array_equal(viol, want['viol'][rows]) and np.array_equal(iters, want['iters'][rows])
    nan = np.isnan(want['post'][rows])                               # (after an overflow; a NaN's sign and payload carry nothing)
    assert np.array_equal(np.isnan(post), nan)
    assert np.array_equal(bits(post)[~nan], bits(want['post'][rows])[~nan])


@pytest.mark.parametrize('name', CODES)
def test_inputs_hold_all_three_kinds(name):
    r = restated(name, 'min-sum', 'flooding', MS_ITERS)
    done, first = r['viol'] == 0, (r['viol'] == 0) & (r['iters'] == 1)
    print(name, 'decoded', int(done.sum()), 'not', int((~done).sum()), 'clean at iteration 1', int(first.sum()))
    assert done.any() and (~done).any() and first.any()
    assert (done & (r['iters'] > 1)).any()


@pytest.mark.parametrize('schedule', SCHEDULES)
@pytest.mark.parametrize('algorithm', ('min-sum', 'offset-min-sum'))
@pytest.mark.parametrize('name', CODES)
def test_min_sum_equals_the_restatement_bit_for_bit(paths, name, algorithm, schedule):
    llr = case(name)[3]
    want = restated(name, algorithm, schedule, MS_ITERS)
    assert_bitwise(run(paths(name), llr, algorithm=algorithm, schedule=schedule, max_iter=MS_ITERS), want)
    assert_bitwise(run(paths(name), llr[:1], algorithm=algorithm, schedule=schedule, max_iter=MS_ITERS), want, slice(0, 1))      # B = 1


@pytest.mark.parametrize('name', CODES)
def test_min_sum_edge_inputs(paths, name):
    code, tabs, layers, llr = case(name)
    N, path = code.n_var, paths(name)
    special = llr[:8].copy()
    special[0, 3 % N], special[1, 5 % N], special[2, 7 % N] = np.nan, 1e9, -1e9             # the load rule: NaN -> 0, clamp to +-4096
    for algorithm, schedule in (('min-sum', 'flooding'), ('min-sum', 'layered'), ('offset-min-sum', 'flooding'),
                                ('offset-min-sum', 'layered')):
        lay = layers if schedule == 'layered' else None
        kw = dict(algorithm=algorithm, schedule=schedule)
        zeros = np.zeros((4, N), np.float32)                                                # ties everywhere, the sign of zero
        want = LO.decode(zeros, tabs, lay, algorithm, 5)
        assert (want['iters'] == 1).all() and not want['x'].any()
        assert_bitwise(run(path, zeros, max_iter=5, **kw), want)
        assert_bitwise(run(path, special, max_iter=MS_ITERS, **kw), LO.decode(special, tabs, lay, algorithm, MS_ITERS))
        one = restated(name, algorithm, schedule, 1)                                        # max_iter = 1
        assert (one['iters'] == 1).all()
        assert_bitwise(run(path, llr, max_iter=1, **kw), one)
        wide = torch.full((B, N + 5), float('nan'), device='cuda')                          # a strided llr: llr_sb = N + 5 > N
        wide[:, :N] = torch.from_numpy(np.array(llr))
        assert wide[:, :N].stride(0) == N + 5
        assert_bitwise(run(path, wide[:, :N], max_iter=MS_ITERS, **kw), restated(name, algorithm, schedule, MS_ITERS))
        assert_bitwise(run(path, llr, max_iter=MS_ITERS, alpha=0.75, beta=0.25, **kw),
                       LO.decode(llr, tabs, lay, algorithm, MS_ITERS, alpha=0.75, beta=0.25))


@pytest.mark.parametrize('max_iter', SP_ITERS)
@pytest.mark.parametrize('schedule', SCHEDULES)
@pytest.mark.parametrize('name', CODES)
def test_sum_product_within_the_restatements_own_error(paths, name, schedule, max_iter):
    llr = case(name, True)[3]
    want = restated(name, 'sum-product', schedule, max_iter, 'float64')
    near = restated(name, 'sum-product', schedule, max_iter)
    keep = want['margin'] > SP_BOUND
    assert (~keep).mean() <= 0.05
    own = float((np.abs(near['post'].astype(np.float64) - want['post']) / np.maximum(1.0, np.abs(want['post']))).max())
    assert own <= SP_D * (1 + 1e-3), own                                        # d is what the docstring says it is
    for rows in (slice(None), slice(0, 1)):                                    # B = 67, B = 1
        x, viol, iters, post = run(paths(name), llr[rows], algorithm='sum-product', schedule=schedule, max_iter=max_iter)
        err = float((np.abs(post.astype(np.float64) - want['post'][rows]) / np.maximum(1.0, np.abs(want['post'][rows])))[keep[rows]].max())
        print(name, schedule, max_iter, 'device error %.3e, restatement f32 error %.3e, bound %.3e, words left out %d'
              % (err, own, SP_BOUND, int((~keep[rows]).sum())))
        assert err <= SP_BOUND
        k = keep[rows]
        assert np.array_equal(x[k], want['x'][rows][k])
        assert np.array_equal(viol[k], want['viol'][rows][k]) and np.array_equal(iters[k], want['iters'][rows][k])


def test_sum_product_zero_llrs_and_the_load_rule(paths):
    code, tabs, layers, llr = case('builtin', True)
    x, viol, iters, post = run(paths('builtin'), np.zeros((3, 96), np.float32), algorithm='sum-product', max_iter=4)
    assert not x.any() and not viol.any() and (iters == 1).all() and not post.any()          # tanh(0) = 0: every message is 0
    special = llr[:8].copy()
    special[0, 3], special[1, 5], special[2, 7] = np.nan, 1e9, -1e9
    for schedule in SCHEDULES:
        want = LO.decode(special, tabs, layers if schedule == 'layered' else None, 'sum-product', 3, dtype=np.float64)
        x, viol, iters, post = run(paths('builtin'), special, algorithm='sum-product', schedule=schedule, max_iter=3)
        keep = want['margin'] > SP_BOUND
        assert keep.sum() >= 6
        err = (np.abs(post - want['post']) / np.maximum(1.0, np.abs(want['post'])))[keep].max()
        assert err <= SP_BOUND, err
        assert np.array_equal(x[keep], want['x'][keep]) and np.array_equal(iters[keep], want['iters'][keep])


def test_decode_llr_takes_the_code_decode_refuses(paths):
    path = paths('g1024')
    with pytest.raises(ValueError, match='edges'):
        path.decode(torch.zeros(1, 1024, dtype=torch.float64, device='cuda'))
    x, viol, iters = path.decode_llr(torch.from_numpy(case('g1024')[3]).cuda(), 'min-sum', 'layered')
    assert x.shape == (B, 1024) and int((viol == 0).sum()) > 0
    assert path.decode_llr(torch.zeros(0, 1024, device='cuda'))[0].shape == (0, 1024)          # B = 0: no launch


def test_a_code_above_48_kib_of_lds():
    """N = 768, M = 384, E = 6144 on 256 threads: the word state (59168 B here, 57632 B in the learned forward) passes the 48 KiB
    a kernel gets without its dynamic-LDS limit raised, which no other code of this file does (g1024: about 46 KB).  Five words at
    4 dB, 10 iterations: in the restatement flooding min-sum decodes four (iterations 3, 4, 4, 4) and leaves one with 8 violated
    checks, the layered schedule decodes all five; no NaN appears."""
    from fgnn_amd import _hip
    from fgnn_amd.datapath import LdpcDataPath
    from fgnn_amd.ldpc_code import LdpcCode
    from fgnn_amd.ldpc_nms import LearnedMinSum
    code = LdpcCode.gallager(768, 8, 16, 1)
    tabs, layers = LO.tables(code.nlist, code.n_chk), code.layers()
    N, M, E = code.n_var, code.n_chk, len(tabs[2])
    assert (N, M, E) == (768, 384, 6144)
    assert int(_hip.invoke('fgnn_ldpc_decode_llr_lds_bytes', N, M, E)) == 59168 > 48 * 1024
    assert int(_hip.invoke('fgnn_ldpc_nms_lds_bytes', N, M, E, 0)) == 57632 > 48 * 1024
    llr = received(code, 7, (4.0, 4.0), 5)
    path = LdpcDataPath('cuda:0', code)
    flooding = None
    for algorithm in ('min-sum', 'offset-min-sum'):
        for schedule in SCHEDULES:
            want = LO.decode(llr, tabs, layers if schedule == 'layered' else None, algorithm, 10)
            assert not np.isnan(want['post']).any()
            if (algorithm, schedule) == ('min-sum', 'flooding'):
                flooding = want
                assert (want['viol'] == 0).any() and (want['viol'] != 0).any()          # decoded and undecoded words
            first = run(path, llr, algorithm=algorithm, schedule=schedule, max_iter=10)
            assert_bitwise(first, want)
            again = run(path, llr, algorithm=algorithm, schedule=schedule, max_iter=10)  # (the limit is raised once: no call now)
            assert all(np.array_equal(a, b) for a, b in zip(first[:3], again[:3])) and np.array_equal(bits(first[3]), bits(again[3]))
    dec = LearnedMinSum(code, 10, 'iteration', alpha=0.8125, beta=0.0).cuda()
    for _ in range(2):
        x, viol, iters, post = dec.decode(torch.from_numpy(np.array(llr)).cuda(), want_posteriors=True)
        assert_bitwise((x.cpu().numpy(), viol.cpu().numpy(), iters.cpu().numpy(), post.cpu().numpy()), flooding)


def test_evaluate_takes_decoder_specs(paths):
    from fgnn_amd import ldpc_eval
    path = paths('builtin')
    ts = path.make_test_set(num=2, baseline=False)
    model = ZeroLogits().cuda()
    res = ldpc_eval.evaluate(model, ts, baseline=['mackay', 'min-sum:layered'])
    old = ldpc_eval.evaluate(model, ts, baseline=True)
    assert 'baseline' not in res and set(res['baselines']) == {'mackay', 'min-sum:layered'}
    assert np.array_equal(res['baselines']['mackay']['counts'], old['baseline']['counts'])
    assert np.array_equal(res['counts'], old['counts'])
    single = ldpc_eval.evaluate(model, ts, baseline='min-sum:layered')
    assert np.array_equal(single['baseline']['counts'], res['baselines']['min-sum:layered']['counts'])
    # the restatement's counts on the same received words
    code, tabs, layers, _ = case('builtin')
    y, gts, snr = ts['noizy_sg'].numpy(), ts['gts'].numpy(), ts['snr_dbs'].numpy()[:, 0]
    llr = path.bit_llr(ts['noizy_sg'], ts['snr_dbs'][:, 0]).cpu().numpy()
    assert llr.dtype == np.float32 and np.allclose(llr, -2.0 * 10.0 ** (snr[:, None].astype(np.float64) / 20.0) * y, rtol=1e-5, atol=0)
    want = LO.decode(llr, tabs, layers, 'min-sum', 50)
    wrong = want['x'][:, :48] != gts[:, :48]
    counts = res['baselines']['min-sum:layered']['counts']
    assert list(counts[-1]) == [48 * len(y), int(wrong.sum()), len(y), int(wrong.any(1).sum())]
    sb = ts['sigma_b'].numpy().astype(np.int64)
    for i, s in enumerate(ldpc_eval.SNR_GRID):
        for j, g in enumerate(ldpc_eval.SIGMA_GRID):
            sel = (np.abs(snr - s) < 1e-3) & (sb == g)
            assert list(counts[i * len(ldpc_eval.SIGMA_GRID) + j]) == [48 * int(sel.sum()), int(wrong[sel].sum()), int(sel.sum()),
                                                                     int(wrong[sel].any(1).sum())]


def test_ber_curve_counts_are_the_restatements():
    from fgnn_amd import ldpc_eval
    from fgnn_amd.datapath import LdpcDataPath
    from fgnn_amd.ldpc_code import LdpcCode
    code = LdpcCode.gallager(24, 3, 6, 0)
    rows = ldpc_eval.ber_curve(code, 'min-sum:layered', snr_db=(2.0,), batch=64, max_words=256, min_word_errors=10 ** 9)
    assert len(rows) == 1 and rows[0]['words'] == 256 and rows[0]['snr_db'] == 2.0            # exactly 4 batches
    path = LdpcDataPath('cuda:0', code)
    path.sigma_b_choices = (0,)
    tabs, layers = LO.tables(code.nlist, code.n_chk), code.layers()
    bit_errors = word_errors = iters = 0
    for j in range(4):
        drawn = path.sample_rng(64, seed=0, step=j, snr_db=2.0)
        assert (drawn.snr_db == 2.0).all() and (drawn.sigma_b == 0).all()
        llr = path.bit_llr(drawn.y, drawn.snr_db).cpu().numpy()
        want = LO.decode(llr, tabs, layers, 'min-sum', 50)
        wrong = want['x'][:, :code.K] != drawn.cw.cpu().numpy()[:, :code.K]
        bit_errors, word_errors, iters = bit_errors + int(wrong.sum()), word_errors + int(wrong.any(1).sum()), iters + int(want['iters'].sum())
    r = rows[0]
    assert (r['bit_errors'], r['word_errors']) == (bit_errors, word_errors)
    assert r['ber'] == bit_errors / (256 * code.K) and r['wer'] == word_errors / 256 and r['mean_iters'] == iters / 256
