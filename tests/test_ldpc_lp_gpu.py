"""GPU: the ADMM linear-programming LDPC decoder (csrc/ldpc_lp.hip; LdpcDecoders.decode_lp, Decoder.run, ldpc_eval.evaluate /
ber_curve) against the numpy restatement tests/ldpc_lp_oracle.py and against brute-force maximum-likelihood decoding.

Inputs and settings: tests/ldpc_lp_cases.py.  The fixed-count cases run with eps = -1 (the residual rule off) and stop_on_codeword =
0; with eps = 0 the two precisions of the restatement themselves stop at different iterations (a word at an integral fixed point has
res = dz = 0 exactly, and f32 gets there first).

The yardstick is the float64 restatement.  d (``LP_D``), the largest |x_f32 - x_f64| between the restatement's own two precisions
over the fixed-count cases (measured on the CPU by ``restatement_error``; the worst is g32, plain, 50 iterations), is 2.671e-06 and
the bound is 4 d = 1.068e-05 (``BOUND``): the device may order nothing differently from the f32 restatement (every operation is an
IEEE add, multiply, divide, minimum, maximum or compare in a fixed order), so its distance to the yardstick is of the size that
separates the two precisions.  soft must lie within the bound; xh, viol, iters and flags must equal the yardstick's on every word
whose decision margin (the smallest |x[n] - 0.5|: at the last iteration, and with stop_on_codeword over the whole run, since every
iteration's decisions then decide the stop) exceeds the bound.  At most 5 % of the words may be left out (asserted).

Stop-rule cases: a word is also left out when its stop or its certificate could fall differently in another precision: the word met
the residual rule and some |min(x, 1 - x) - 1e-3| is within the bound, or at some iteration r = max(res, dz) is within ``R_BOUND`` of
eps.  The issue that asked for this decoder set that second tolerance to the bound too; 4 d = 1.07e-5 exceeds eps = 1e-5 itself, so
every word that converges (r falls to zero) would be left out and the 5 % cap could not hold on any input.  r near eps is a
difference of nearly equal x and z, far more exact than x itself: d_r (``LP_D_R``), the largest |r_f32 - r_f64| between the
restatement's two precisions over the iterations of the stop-rule cases at which r_f64 <= 2 eps, is 1.413e-07, and ``R_BOUND`` = 4 d_r
by the same margin.  r = 0 is exempt: it arises only from x and z that are all clipped to 0 or 1, exact in every precision (an integral
optimum is reached exactly, which is why the rule is stable).  This leaves out fewer words than the issue's wording, so it asks
more of the device, not less."""
import functools

import numpy as np
import pytest
import torch

import ldpc_lp_cases as C
import ldpc_lp_oracle as LP
from ldpc_decoder_cases import ZeroLogits, make_paths

pytestmark = pytest.mark.gpu

LP_D = 2.671e-06            # measured: restatement_error()[0] (module docstring)
LP_D_R = 1.413e-07          # measured: restatement_error()[1]
BOUND = 4 * LP_D
R_BOUND = 4 * LP_D_R
LEFT_OUT_CAP = 0.05
STOP_NAMES = C.CODES + ('irregular', 'g768')


def restatement_error():
    """(d, d_r) of the module docstring; run on the CPU (test_ldpc_lp.py asserts the constants above against it)."""
    d = max(C.soft_error(C.restated(name, key)['soft'], C.restated(name, key, 'float64')['soft']) for name, key in C.fixed_cases())
    d_r = 0.0
    for name in STOP_NAMES:
        for key in C.STOP:
            a, b = C.restated(name, key)['r'], C.restated(name, key, 'float64')['r']
            at = ~np.isnan(a) & ~np.isnan(b) & (b <= 2 * C.STOP[key]['eps'])
            d_r = max(d_r, float(np.abs(a - b)[at].max()) if at.any() else 0.0)
    return d, d_r


@functools.lru_cache(maxsize=None)
def yardstick(name, key):
    """(the f64 restatement with its ``near`` at the tolerances above, the words compared [B] bool)."""
    want = C.restated(name, key, 'float64', BOUND, R_BOUND)
    soc = C.SETTINGS[key]['stop_on_codeword']
    keep = (want['margin_run' if soc else 'margin'] > BOUND) & ~want['near']
    return want, keep


paths = pytest.fixture(scope='module', name='paths')(make_paths)


@functools.lru_cache(maxsize=None)
def device_tables(name):
    return tuple(torch.from_numpy(np.asarray(t, np.int32)).cuda() for t in C.case(name)[0])


def run(paths, name, llr, **kw):
    """(x, soft, viol, iters, flags) as numpy arrays: through ``decode_lp`` for an ``LdpcCode``, through the C entry point for the
    hand-made tables (and for g768, whose path would be one more object to build)."""
    from fgnn_amd import _hip
    if not isinstance(llr, torch.Tensor):
        llr = torch.from_numpy(np.array(llr, np.float32)).cuda()
    if name in C.CODES:
        x, viol, iters, flags, soft = paths(name).decode_lp(llr, want_soft=True, **kw)
    else:
        col_ptr, row_ptr, row_edge, row_var = device_tables(name)
        n, N = llr.shape
        x, soft = torch.empty((n, N), dtype=torch.uint8, device='cuda'), torch.empty((n, N), device='cuda')
        viol, iters, flags = (torch.empty(n, dtype=torch.int32, device='cuda') for _ in range(3))
        _hip.call('fgnn_ldpc_decode_lp', llr, llr.stride(0), col_ptr, row_ptr, row_edge, row_var, n, N, len(row_ptr) - 1, len(row_edge),
                  kw['max_iter'], kw['mu'], kw['penalty'], kw['relax'], kw['eps'], kw['stop_on_codeword'], x, soft, viol, iters, flags)
    return tuple(t.cpu().numpy() for t in (x, soft, viol, iters, flags))


def assert_matches(got, want, keep, rows=slice(None), what=''):
    x, soft, viol, iters, flags = got
    k = keep[rows]
    err = C.soft_error(soft[k], want['soft'][rows][k]) if k.any() else 0.0
    print(what, 'device error %.3e, bound %.3e, words left out %d of %d' % (err, BOUND, int((~k).sum()), len(k)))
    assert err <= BOUND
    assert np.array_equal(x[k], want['x'][rows][k])
    assert np.array_equal(viol[k], want['viol'][rows][k]) and np.array_equal(iters[k], want['iters'][rows][k])
    assert np.array_equal(flags[k], want['flags'][rows][k])


def compare(paths, name, key):
    want, keep = yardstick(name, key)
    assert (~keep).mean() <= LEFT_OUT_CAP, int((~keep).sum())
    llr = C.case(name)[1]
    for rows in (slice(None), slice(0, 1)):                            # B = 67 (5 for g768), B = 1
        assert_matches(run(paths, name, llr[rows], **C.SETTINGS[key]), want, keep, rows, '%s %s' % (name, key))


@pytest.mark.parametrize('name,key', C.fixed_cases())
def test_fixed_count_within_the_restatements_own_error(paths, name, key):
    own = C.soft_error(C.restated(name, key)['soft'], C.restated(name, key, 'float64')['soft'])
    assert own <= LP_D * (1 + 1e-3), own                               # d is what the docstring says it is
    want, _ = yardstick(name, key)
    assert (want['iters'] == C.FIXED[key]['max_iter']).all() and not want['flags'].any()          # a fixed count: no rule stops a word
    compare(paths, name, key)


@pytest.mark.parametrize('key', list(C.STOP))
@pytest.mark.parametrize('name', STOP_NAMES)
def test_stop_rules_within_the_restatements_own_error(paths, name, key):
    compare(paths, name, key)


@pytest.mark.parametrize('key', list(C.STOP))
@pytest.mark.parametrize('name', C.CODES)
def test_stop_rule_inputs_hold_all_three_kinds(name, key):
    want, _ = yardstick(name, key)
    last = C.STOP[key]['max_iter']
    stopped = (want['flags'] & 1).astype(bool) | ((want['viol'] == 0) & (want['iters'] < last) if key == 'pen-stop' else False)
    print(name, key, 'stopped', int(stopped.sum()), 'ran out', int((~stopped).sum()), 'stopped after iteration 1', int((stopped & (want['iters'] > 1)).sum()))
    assert stopped.any() and (~stopped).any() and (stopped & (want['iters'] > 1)).any()
    assert (want['iters'][~stopped] == last).all()


@pytest.mark.parametrize('name', C.CODES)
def test_strided_llr_the_load_rule_and_repeatability(paths, name):
    tabs, llr = C.case(name)
    N = llr.shape[1]
    for key in ('plain-r1.9-i8', 'pen-stop'):
        want, keep = yardstick(name, key)
        wide = torch.full((C.B, N + 5), float('nan'), device='cuda')                        # a strided llr: llr_sb = N + 5, NaN in the padding
        wide[:, :N] = torch.from_numpy(np.array(llr))
        assert wide[:, :N].stride(0) == N + 5
        first = run(paths, name, wide[:, :N], **C.SETTINGS[key])
        assert_matches(first, want, keep, what='%s %s strided' % (name, key))
        again = run(paths, name, llr, **C.SETTINGS[key])                                    # two calls, the same bits
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(first, again))
    special = llr[:8].copy()
    special[0, 3 % N], special[1, 5 % N], special[2, 7 % N] = np.nan, 1e9, -1e9             # the load rule: NaN -> 0, clamp to +-4096
    kw = C.SETTINGS['plain-r1.9-i8']
    want = LP.decode(special, tabs, dtype=np.float64, **kw)
    keep = want['margin'] > BOUND
    assert keep.sum() >= 6
    assert_matches(run(paths, name, special, **kw), want, keep, what='%s load rule' % name)
    clamped = np.clip(np.where(np.isnan(special), 0, special), -4096, 4096).astype(np.float32)
    assert np.array_equal(LP.decode(clamped, tabs, dtype=np.float64, **kw)['soft'], want['soft'])


@pytest.mark.parametrize('which,snr', C.CERTIFICATE_CASES)
def test_certified_words_are_maximum_likelihood(which, snr):
    """The independent check of the projection and the stop rule: the device's certified words against enumeration."""
    from fgnn_amd.datapath import LdpcDataPath
    from fgnn_amd.ldpc_code import LdpcCode
    from ldpc_decoder_cases import code as named_code
    path = LdpcDataPath('cuda:0', named_code('g12') if which == 'g12' else LdpcCode.gallager(24, 3, 6, 0))
    llr = torch.from_numpy(np.array(C.certificate_case(which, snr)[1])).cuda()
    x, viol, iters, flags, soft = (t.cpu().numpy() for t in path.decode_lp(llr, want_soft=True, **C.CERTIFICATE))
    n = C.assert_certified_words_are_ml(which, snr, x, soft, viol, flags)
    print(which, snr, 'certified', n, 'of', len(x))


def test_edges(paths):
    from fgnn_amd import _hip
    from fgnn_amd.datapath import LdpcDataPath
    from fgnn_amd.ldpc_code import LdpcCode
    path = paths('builtin')
    x, viol, iters, flags, soft = path.decode_lp(torch.zeros(3, 96, device='cuda'), want_soft=True)         # all-zero LLRs
    assert (soft == 0.5).all() and (iters == 1).all() and (flags == 1).all() and not x.any()
    out = path.decode_lp(torch.zeros(0, 96, device='cuda'), want_soft=True)                                  # B = 0: no launch
    assert [tuple(t.shape) for t in out] == [(0, 96), (0,), (0,), (0,), (0, 96)]
    big = LdpcCode.gallager(1024, 16, 16, 0)                                                                  # E = 16384: refused
    assert int(_hip.invoke('fgnn_ldpc_decode_lp_lds_bytes', 1024, 1024, 16384)) < 0
    with pytest.raises(ValueError, match='LDS'):
        LdpcDataPath('cuda:0', big).decode_lp(torch.zeros(1, 1024, device='cuda'))
    assert int(_hip.invoke('fgnn_ldpc_decode_lp_lds_bytes', 768, 384, 6144)) > 48 * 1024                     # g768 (compared above)
    with pytest.raises(ValueError, match='smallest variable degree'):
        path.decode_lp(torch.zeros(1, 96, device='cuda'), mu=1.0, penalty=1.5)


def test_decoder_spec_runs_and_osd_returns_codewords(paths):
    from fgnn_amd.ldpc_decoders import parse_decoder
    path, code = paths('builtin'), C.named_code('builtin')
    rng = np.random.RandomState(11)
    snr = np.full(C.B, 1.0, np.float32)
    y = torch.from_numpy((-10.0 ** (1.0 / 20.0) + rng.standard_normal((C.B, 96))).astype(np.float32)).cuda()
    plain = parse_decoder('admm-lp:iters=100').run(path, y, torch.from_numpy(snr).cuda())
    assert len(plain) == 3 and (plain[1] != 0).any()                                       # some words are left with violated checks
    x, viol, iters = parse_decoder('admm-lp:iters=100:osd=1').run(path, y, torch.from_numpy(snr).cuda())
    H = C.parity_matrix(code).astype(np.int64)
    assert not ((x.cpu().numpy().astype(np.int64) @ H.T) % 2).any() and not viol.any()
    assert torch.equal(iters, plain[2])
    done = plain[1] == 0
    assert torch.equal(x[done], plain[0][done])                                            # a decoded word passes through


def test_evaluate_and_ber_curve_count_certificates(paths):
    """The pattern of test_ldpc_llr_gpu.py's test_ber_curve_counts_are_the_restatements: gallager(24, 3, 6, 0), 4 batches of 64."""
    from fgnn_amd import ldpc_eval
    from fgnn_amd.datapath import LdpcDataPath
    from fgnn_amd.ldpc_code import LdpcCode
    import ldpc_llr_oracle as LO
    code = LdpcCode.gallager(24, 3, 6, 0)
    spec = 'admm-lp:iters=100'
    rows = ldpc_eval.ber_curve(code, spec, snr_db=(2.0,), batch=64, max_words=256, min_word_errors=10 ** 9)
    assert len(rows) == 1 and rows[0]['words'] == 256
    path = LdpcDataPath('cuda:0', code)
    path.sigma_b_choices = (0,)
    tabs = LO.tables(code.nlist, code.n_chk)
    tot = dict(bit_errors=0, word_errors=0, iters=0, ml_certified=0, certified_word_errors=0)
    left_out = 0
    for j in range(4):
        drawn = path.sample_rng(64, seed=0, step=j, snr_db=2.0)
        llr = path.bit_llr(drawn.y, drawn.snr_db).cpu().numpy()
        want = LP.decode(llr, tabs, max_iter=100, dtype=np.float64, tol=BOUND, tol_r=R_BOUND)
        left_out += int(((want['margin'] <= BOUND) | want['near']).sum())
        cw = drawn.cw.cpu().numpy()
        wrong = want['x'][:, :code.K] != cw[:, :code.K]
        cert = (want['flags'] & 2) != 0
        tot['bit_errors'] += int(wrong.sum())
        tot['word_errors'] += int(wrong.any(1).sum())
        tot['iters'] += int(want['iters'].sum())
        tot['ml_certified'] += int(cert.sum())
        tot['certified_word_errors'] += int((cert & (want['x'] != cw).any(1)).sum())
    r = rows[0]
    print('ber_curve', {k: r[k] for k in tot if k != 'iters'}, 'restatement', tot, 'words left out', left_out)
    assert left_out <= LEFT_OUT_CAP * 256     # a word near a decision may fall either way: it moves a count by at most one (24 per word for bits)
    for k in ('word_errors', 'ml_certified', 'certified_word_errors'):
        assert abs(r[k] - tot[k]) <= left_out, k
    assert abs(r['bit_errors'] - tot['bit_errors']) <= code.K * left_out and abs(r['mean_iters'] * 256 - tot['iters']) <= 100 * left_out
    assert r['ml_certified'] >= 128
    assert 'ml_certified' not in ldpc_eval.ber_curve(code, 'admm-lp:penalty=0.8', snr_db=(2.0,), batch=64, max_words=64, min_word_errors=10 ** 9)[0]
    # evaluate: the same counts through a test set
    bpath = paths('builtin')
    ts = bpath.make_test_set(num=2, baseline=False)
    res = ldpc_eval.evaluate(ZeroLogits().cuda(), ts, baseline=['admm-lp', 'admm-lp:penalty=0.8', 'min-sum:layered'])
    lp = res['baselines']['admm-lp']
    assert 'ml_certified' not in res['baselines']['admm-lp:penalty=0.8'] and 'ml_certified' not in res['baselines']['min-sum:layered']
    llr = bpath.bit_llr(ts['noizy_sg'], ts['snr_dbs'][:, 0]).cpu().numpy()
    want = LP.decode(llr, C.case('builtin')[0], dtype=np.float64, tol=BOUND, tol_r=R_BOUND)
    keep = (want['margin'] > BOUND) & ~want['near']
    gts = ts['gts'].numpy()
    cert = (want['flags'] & 2) != 0
    wrong = (want['x'] != gts).any(1)
    # the words left out may fall either way; every other word counts as the yardstick says
    assert abs(lp['ml_certified'] - int(cert.sum())) <= int((~keep).sum())
    assert abs(lp['certified_word_errors'] - int((cert & wrong).sum())) <= int((~keep).sum())
    assert (~keep).mean() <= LEFT_OUT_CAP and lp['ml_certified'] > 0
    single = ldpc_eval.evaluate(ZeroLogits().cuda(), ts, baseline='admm-lp')
    assert single['baseline']['ml_certified'] == lp['ml_certified'] and np.array_equal(single['baseline']['counts'], lp['counts'])
