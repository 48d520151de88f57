"""CPU: the ADMM linear-programming LDPC decoder's checker and host side (csrc/ldpc_lp.hip, include/fgnn_hip_ldpc_lp.h,
LdpcDecoders.decode_lp, ldpc_decoders.parse_decoder).

  * the companion header binds beside the main one, whose interface is what it was;
  * the byte query and the argument validation of the entry point happen before any launch, so they are testable without a device;
  * the restatement tests/ldpc_lp_oracle.py: its projection satisfies the variational inequality of a Euclidean projection against
    every vertex of the parity polytope, and the words it certifies are the maximum-likelihood codewords found by enumeration;
  * the constants test_ldpc_lp_gpu.py compares the device with are what the restatement gives."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import ldpc_llr_oracle as LO
import ldpc_lp_cases as C
import ldpc_lp_oracle as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANION = os.path.join(ROOT, 'include', 'fgnn_hip_ldpc_lp.h')
NEW = ('fgnn_ldpc_decode_lp', 'fgnn_ldpc_decode_lp_lds_bytes')
EINVAL = -1                                    # FGNN_EINVAL


def test_companion_header_is_parsed_bound_and_built():
    from fgnn_amd import _hip
    text = open(COMPANION).read()
    assert '#include "fgnn_hip.h"' in text and 'extern "C"' in text
    sig = _hip.signatures(text)
    assert tuple(sig) == NEW == _hip.LDPC_LP
    assert not set(NEW) & set(_hip.EXPORTS) and not set(NEW) & set(_hip.SIGNATURES) and _hip.ABI_VERSION == 15
    main = open(_hip.HEADER_PATH).read()
    assert not any(re.search(r'\b%s\b' % name, main) for name in NEW)
    L = _hip.lib()
    for name in NEW:
        fn = getattr(L, name)                                        # exported by the built library ...
        restype, params = sig[name]
        assert fn.restype is restype                                 # ... and bound with the parsed types
        assert list(fn.argtypes) == [t for _, t in params] and _hip.COMPANIONS[name][:2] == sig[name]
    assert sig[NEW[0]][0] is ctypes.c_int32 and sig[NEW[1]][0] is ctypes.c_int64
    assert [n for n, _ in sig[NEW[0]][1]] == ['llr', 'llr_sb', 'col_ptr', 'row_ptr', 'row_edge', 'row_var', 'B', 'N', 'M', 'E', 'max_iter',
                                              'mu', 'penalty', 'relax', 'eps', 'stop_on_codeword', 'x', 'soft', 'viol', 'iters', 'flags',
                                              'stream']
    args = dict(sig[NEW[0]][1])
    assert all(args[k] is ctypes.c_float for k in ('mu', 'penalty', 'relax', 'eps')) and args['B'] is ctypes.c_int64
    assert args['llr_sb'] is ctypes.c_int64 and args['llr'] is _hip.DevicePointer and args['stream'] is _hip.DevicePointer
    assert [n for n, _ in sig[NEW[1]][1]] == ['N', 'M', 'E']
    assert text.count('No counterpart in the reference') == 2        # each prototype says why it exists
    assert 'THE CALLER guarantees' in text                           # 2 penalty / mu < the smallest variable degree


def test_library_footprint_and_validation_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    q = lambda n, m, e: int(_hip.invoke('fgnn_ldpc_decode_lp_lds_bytes', n, m, e))
    # per word: f32 z [E], x [N], g [N]; the packed row table [E]; 16 scratch words; 16-bit row_ptr, col_ptr padded to a word; f32 u [E]
    want = lambda n, m, e: (4 * (2 * e + 2 * n) + 64 + (2 * ((m + 1) + (n + 1)) + 3) // 4 * 4 + 4 * e + 15) // 16 * 16
    for n, m, e in ((96, 48, 288), (12, 6, 36), (1024, 512, 4096), (768, 384, 6144), (1, 1, 1), (6, 5, 12)):
        assert q(n, m, e) == want(n, m, e), (n, m, e)
    assert q(96, 48, 288) < 8192 and q(768, 384, 6144) > 48 * 1024
    sizes = [q(1024, 1024, e) for e in range(1024, 12289, 512)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[-1] <= 160 * 1024          # grows with E
    assert q(1024, 1024, 16384) == -1 and b'LDS' in L.fgnn_last_error()                     # the E = 16384 corner no longer fits 160 KiB
    assert want(1024, 1024, 16384) > 160 * 1024
    fits = max(e for e in range(12288, 16385, 16) if want(1024, 1024, e) <= 160 * 1024)     # the boundary is the formula's
    assert q(1024, 1024, fits) == want(1024, 1024, fits) and q(1024, 1024, fits + 16) == -1
    for n, m, e in ((1025, 48, 288), (0, 48, 288), (96, 1025, 288), (96, 0, 288), (96, 48, 0), (96, 48, -1), (96, 48, 16 * 48 + 1),
                    (8, 48, 16 * 8 + 1)):
        assert q(n, m, e) == -1, (n, m, e)
    assert b'variables' in (q(1025, 48, 288), L.fgnn_last_error())[1]
    assert b'checks' in (q(96, 1025, 288), L.fgnn_last_error())[1]
    assert b'edges' in (q(96, 48, 769), L.fgnn_last_error())[1]

    one = ctypes.c_void_p(16)                      # a non-NULL pointer that is never dereferenced on these paths
    def dec(llr=one, sb=96, tab=one, B=4, n=96, m=48, e=288, it=50, mu=3.0, penalty=0.0, relax=1.9, eps=1e-5, soc=0, x=one, viol=one,
            iters=one, flags=one):
        return _hip.invoke('fgnn_ldpc_decode_lp', llr, sb, tab, tab, tab, tab, B, n, m, e, it, mu, penalty, relax, eps, soc, x, None, viol,
                           iters, flags, None)
    assert dec(n=1025) == _hip.EUNSUPPORTED and dec(m=1025) == _hip.EUNSUPPORTED and dec(e=16 * 48 + 1) == _hip.EUNSUPPORTED
    assert dec(n=0) == _hip.EUNSUPPORTED and dec(e=0) == _hip.EUNSUPPORTED
    assert dec(n=1024, m=1024, e=16384) == _hip.EUNSUPPORTED and b'LDS' in L.fgnn_last_error()
    assert dec(it=0) == EINVAL and b'max_iter' in L.fgnn_last_error()
    for v in (0.0, -1.0, float('nan'), float('inf')):
        assert dec(mu=v) == EINVAL and b'mu' in L.fgnn_last_error()
    for v in (-0.5, float('nan'), float('inf')):
        assert dec(penalty=v) == EINVAL and b'penalty' in L.fgnn_last_error()
    for v in (0.99, 2.0, -1.0, float('nan'), float('inf')):
        assert dec(relax=v) == EINVAL and b'relax' in L.fgnn_last_error()
    for v in (float('nan'), float('inf'), -float('inf')):
        assert dec(eps=v) == EINVAL and b'eps' in L.fgnn_last_error()
    assert dec(soc=2) == EINVAL and dec(soc=-1) == EINVAL and b'stop_on_codeword' in L.fgnn_last_error()
    assert dec(sb=-1) == EINVAL and b'stride' in L.fgnn_last_error()
    assert dec(B=-1) == EINVAL and dec(B=2 ** 31) == EINVAL and b'batch' in L.fgnn_last_error()
    assert dec(llr=None) == EINVAL and dec(tab=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert dec(x=None) == EINVAL and dec(viol=None) == EINVAL and dec(iters=None) == EINVAL and dec(flags=None) == EINVAL
    assert dec(llr=None, tab=None, x=None, viol=None, iters=None, flags=None, B=0) == 0            # empty batch: nothing to do
    assert dec(B=0, eps=-1.0, relax=1.0, soc=1) == 0                                               # eps < 0: the residual rule off
    assert dec(B=0, n=1025) == _hip.EUNSUPPORTED and dec(B=0, it=0) == EINVAL                      # sizes are checked even then


# decoder specs -> parse_decoder's (canonical spec, kind, arguments), and specs it refuses: the shape of test_ldpc_llr.py's tables
DEFAULTS = dict(max_iter=200, mu=3.0, penalty=0.0, relax=1.9, eps=1e-5)
PARSED = (
    ('admm-lp', 'admm-lp', 'lp', DEFAULTS),
    ('admm-lp:iters=200:mu=3:penalty=0:relax=1.9:eps=1e-5', 'admm-lp', 'lp', DEFAULTS),
    ('admm-lp:penalty=0.8', 'admm-lp:penalty=0.8', 'lp', dict(DEFAULTS, penalty=0.8)),
    ('admm-lp:iters=50:mu=2.5:penalty=1.5:relax=1:eps=0.001', 'admm-lp:iters=50:mu=2.5:penalty=1.5:relax=1.0:eps=0.001', 'lp',
     dict(max_iter=50, mu=2.5, penalty=1.5, relax=1.0, eps=0.001)),
    ('admm-lp:eps=-1', 'admm-lp:eps=-1.0', 'lp', dict(DEFAULTS, eps=-1.0)),
    ('admm-lp:osd=1', 'admm-lp:osd=1', 'lp', dict(DEFAULTS, osd=1)),
    ('admm-lp:penalty=0.8:osd=2:span=32', 'admm-lp:penalty=0.8:osd=2:span=32', 'lp', dict(DEFAULTS, penalty=0.8, osd=2, span=32)),
    ('admm-lp:iters=30:osd=0', 'admm-lp:iters=30:osd=0', 'lp', dict(DEFAULTS, max_iter=30, osd=0)))
JUNK = ('admm-lp:', 'admm-lp:layered', 'admm-lp:flooding', 'admm-lp:iters=0', 'admm-lp:iters=x', 'admm-lp:iters=2:iters=3', 'admm-lp:mu=0',
        'admm-lp:mu=-1', 'admm-lp:mu=nan', 'admm-lp:mu=inf', 'admm-lp:penalty=-0.1', 'admm-lp:penalty=nan', 'admm-lp:relax=0.9',
        'admm-lp:relax=2', 'admm-lp:relax=nan', 'admm-lp:eps=nan', 'admm-lp:eps=inf', 'admm-lp:alpha=0.5', 'admm-lp:beta=0.5',
        'admm-lp:osd=3', 'admm-lp:span=5', 'admm-lp:osd=0:span=5', 'admm-lp:osd=2:span=257', 'admm-lp:iters', 'admm-lps', 'admm')


def test_parse_decoder_round_trips_and_refuses_junk():
    from fgnn_amd.ldpc_decoders import LLR_ALGORITHMS, LP_DEFAULTS, parse_decoder
    assert LP_DEFAULTS == DEFAULTS and 'admm-lp' not in LLR_ALGORITHMS and len(LLR_ALGORITHMS) == 3
    for spec, canon, kind, kw in PARSED:
        got = parse_decoder(spec)
        assert got == (canon, kind, kw), spec
        assert parse_decoder(canon) == got                                  # the canonical spec parses to itself
        assert got.certifies == (kw['penalty'] == 0)
    for junk in JUNK:
        with pytest.raises(ValueError):
            parse_decoder(junk)
    assert not parse_decoder('min-sum:layered').certifies and not parse_decoder('mackay').certifies


def test_check_decode_lp_args():
    import torch
    from fgnn_amd.ldpc_decoders import check_decode_lp_args
    llr = torch.zeros(5, 96)
    ok = dict(llr=llr, n_var=96, min_degree=3, max_iter=200, mu=3.0, penalty=0.0, relax=1.9, eps=1e-5, stop_on_codeword=None)
    assert check_decode_lp_args(**ok) == (5, 0)
    assert check_decode_lp_args(**dict(ok, penalty=0.8)) == (5, 1)                        # None: penalty > 0
    assert check_decode_lp_args(**dict(ok, penalty=0.8, stop_on_codeword=False)) == (5, 0)
    assert check_decode_lp_args(**dict(ok, stop_on_codeword=True, eps=-1.0, relax=1.0, llr=torch.zeros(0, 96, dtype=torch.float64))) == (0, 1)
    assert check_decode_lp_args(**dict(ok, mu=1.0, penalty=1.49)) == (5, 1)               # 2.98 < 3
    for kw, what in (({'max_iter': 0}, 'max_iter'), ({'max_iter': 2.5}, 'max_iter'), ({'max_iter': True}, 'max_iter'),
                     ({'max_iter': 2 ** 31}, 'max_iter'), ({'mu': 0}, 'mu'), ({'mu': -1.0}, 'mu'), ({'mu': float('nan')}, 'mu'),
                     ({'mu': float('inf')}, 'mu'), ({'penalty': -0.1}, 'penalty'), ({'penalty': float('nan')}, 'penalty'),
                     ({'penalty': 1e39}, 'penalty'), ({'relax': 0.99}, 'relax'), ({'relax': 2.0}, 'relax'), ({'relax': float('nan')}, 'relax'),
                     ({'eps': float('nan')}, 'eps'), ({'eps': float('inf')}, 'eps'), ({'stop_on_codeword': 2}, 'stop_on_codeword'),
                     ({'stop_on_codeword': 'yes'}, 'stop_on_codeword'), ({'mu': 1.0, 'penalty': 1.5}, 'smallest variable degree'),
                     ({'penalty': 3.0, 'min_degree': 2}, 'smallest variable degree'),
                     ({'llr': torch.zeros(5, 95)}, 'llr'), ({'llr': torch.zeros(96)}, 'llr'), ({'llr': np.zeros((5, 96))}, 'llr'),
                     ({'llr': torch.zeros(5, 96, dtype=torch.int32)}, 'floating')):
        with pytest.raises(ValueError, match=what):
            check_decode_lp_args(**dict(ok, **kw))


def test_decode_lp_validates_before_the_device():
    import torch
    from fgnn_amd.datapath import LdpcDataPath
    from fgnn_amd.ldpc_code import LdpcCode
    path = LdpcDataPath.__new__(LdpcDataPath)                                # host side only: no device is touched
    path.N, path.device, path.code = 96, torch.device('cuda:0'), LdpcCode.builtin()
    with pytest.raises(ValueError, match='relax'):
        path.decode_lp(torch.zeros(2, 96), relax=2.0)
    with pytest.raises(ValueError, match='llr'):
        path.decode_lp(torch.zeros(2, 97))
    with pytest.raises(ValueError, match='smallest variable degree, 3'):
        path.decode_lp(torch.zeros(2, 96), mu=1.0, penalty=1.5)
    big = LdpcDataPath.__new__(LdpcDataPath)                                 # E = 16384: the byte query refuses it on the host
    big.code = LdpcCode.gallager(1024, 16, 16, 0)
    big.N, big.device, big._gated, big._tables = 1024, torch.device('cuda:0'), set(), None
    with pytest.raises(ValueError, match='LDS'):
        big.decode_lp(torch.zeros(1, 1024))
    from fgnn_amd.ldpc_eval import evaluate
    with pytest.raises(ValueError, match='decoder'):
        evaluate(torch.nn.Linear(1, 1), {}, baseline=['admm-lp:layered'])


def test_projection_is_the_euclidean_projection():
    """z = P(w) lies in the parity polytope (every odd-set inequality holds) and (w - z) . (v - z) <= 0 for every even-weight vertex v:
    together these characterise the Euclidean projection onto a convex polytope.  f64 to 1e-12, f32 to 1e-5."""
    rng = np.random.RandomState(0)
    for d in (1, 2, 3, 4, 6, 8):
        w = np.concatenate([rng.uniform(-0.7, 1.7, (200, d)), rng.uniform(0.3, 0.7, (100, d)), np.full((1, d), 0.5), np.zeros((1, d)),
                            np.ones((1, d))])
        verts = np.array([v for v in itertools.product((0.0, 1.0), repeat=d) if sum(v) % 2 == 0])
        odd = np.array([v for v in itertools.product((0.0, 1.0), repeat=d) if sum(v) % 2 == 1])
        for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-5)):
            z = LP.project(w.astype(dtype)).astype(np.float64)
            assert z.dtype == np.float64 and (z >= 0).all() and (z <= 1).all()
            theta = 2 * odd - 1
            assert (z @ theta.T - (odd.sum(1) - 1) <= tol).all()                                  # inside
            gap = np.einsum('bd,bvd->bv', w - z, verts[None] - z[:, None])
            assert gap.max() <= tol * (1 + np.abs(w).max()) * d, (d, gap.max())                 # no vertex lies on w's side of z
            assert np.abs(LP.project(z.astype(dtype)) - z).max() <= tol                           # idempotent
        assert np.array_equal(LP.project(verts), verts)
    assert np.array_equal(LP.project(np.array([[0.3], [0.9], [-2.0]])), np.zeros((3, 1)))         # degree 1: z = 0


@pytest.mark.parametrize('which,snr', C.CERTIFICATE_CASES)
def test_certified_words_are_maximum_likelihood(which, snr):
    tabs, llr, _ = C.certificate_case(which, snr)
    for dtype in (np.float32, np.float64):
        r = LP.decode(llr, tabs, dtype=dtype, **C.CERTIFICATE)
        n = C.assert_certified_words_are_ml(which, snr, r['x'], r['soft'], r['viol'], r['flags'])
        print(which, snr, dtype.__name__, 'certified', n, 'of', len(llr))


def test_restatement_properties():
    tabs, llr = C.case('builtin')
    r = LP.decode(np.zeros((3, 96), np.float32), tabs)                                    # all-zero LLRs: the centre is a fixed point
    assert (r['soft'] == 0.5).all() and (r['iters'] == 1).all() and (r['flags'] == 1).all() and not r['x'].any()
    a, b = LP.decode(llr, tabs, max_iter=5, eps=-1.0), LP.decode(llr, tabs, max_iter=5, eps=-1.0, dtype=np.float64)
    assert a['soft'].dtype == np.float32 and b['soft'].dtype == np.float64 and (a['iters'] == 5).all() and not a['flags'].any()
    assert np.abs(a['soft'] - b['soft']).max() <= 1e-5 and np.array_equal(b['margin'], np.abs(b['soft'] - 0.5).min(1))
    # stop_on_codeword: a word stops at its first iteration without a violated check; None reads as penalty > 0
    soc = LP.decode(llr, tabs, max_iter=30, penalty=0.8)
    assert np.array_equal(soc['iters'], LP.decode(llr, tabs, max_iter=30, penalty=0.8, stop_on_codeword=True)['iters'])
    free = LP.decode(llr, tabs, max_iter=30, penalty=0.8, stop_on_codeword=False)
    assert (soc['iters'] <= free['iters']).all() and (soc['iters'] < free['iters']).any()
    assert ((soc['viol'] == 0) | (soc['iters'] == 30) | (soc['flags'] & 1 == 1)).all()
    # the hand-made matrix: its degree-1 check {5} forces x[5] = 0 in every certified word
    itabs, illr = C.case('irregular')
    assert sorted(np.diff(itabs[1])) == [1, 2, 3, 3, 3]
    r = LP.decode(illr, itabs, max_iter=300, relax=1.0, dtype=np.float64)
    cert = (r['flags'] & 2) != 0
    assert cert.sum() >= 40 and not r['x'][cert][:, 5].any() and not r['viol'][cert].any()
    H = np.zeros((5, 6), np.int64)
    H[itabs[1].searchsorted(np.arange(len(itabs[3])), 'right') - 1, itabs[3]] = 1
    cw = C.codewords(H.astype(np.uint8))
    ml = cw[(illr.astype(np.float64) @ cw.T.astype(np.float64)).argmin(1)]
    assert np.array_equal(r['x'][cert], ml[cert])
    # a variable of degree 0 takes its hard decision
    ztabs = LO.tables(np.array([[0], [0], [-1]]), 1)
    r = LP.decode(np.array([[1.0, 2.0, -0.5], [1.0, 2.0, 0.5]], np.float32), ztabs, max_iter=3)
    assert list(r['soft'][:, 2]) == [1.0, 0.0]


def test_the_yardsticks_are_what_the_gpu_file_says():
    import test_ldpc_lp_gpu as G
    d, d_r = G.restatement_error()
    print('d = %.4e, d_r = %.4e' % (d, d_r))
    assert abs(d - G.LP_D) <= 1e-3 * G.LP_D and abs(d_r - G.LP_D_R) <= 1e-3 * G.LP_D_R
    assert G.BOUND == 4 * G.LP_D and G.R_BOUND == 4 * G.LP_D_R
    left = {(name, key): int((~G.yardstick(name, key)[1]).sum()) for name in G.STOP_NAMES for key in C.STOP}
    left.update({case: int((~G.yardstick(*case)[1]).sum()) for case in C.fixed_cases()})
    print('words left out:', {k: v for k, v in left.items() if v})
    assert all(v <= G.LEFT_OUT_CAP * len(C.case(name)[1]) for (name, _), v in left.items())
    # the f32 restatement itself passes the comparison the device is held to
    for name, key in list(left):
        want, keep = G.yardstick(name, key)
        near = C.restated(name, key)
        assert C.soft_error(near['soft'][keep], want['soft'][keep]) <= G.BOUND
        for k in ('x', 'viol', 'iters', 'flags'):
            assert np.array_equal(near[k][keep], want[k][keep]), (name, key, k)
