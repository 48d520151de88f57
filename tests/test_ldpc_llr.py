"""CPU: the LLR-domain LDPC decoders' checker and host side (csrc/ldpc_llr.hip, include/fgnn_hip_ldpc_llr.h, LdpcDataPath.decode_llr,
LdpcCode.layers, ldpc_eval.parse_decoder).

  * the companion header binds beside the main one, whose interface is what it was;
  * argument validation of both entry points happens before any launch, so it is testable without a device;
  * the layers are a partition with no shared variable inside a layer; the LLR decoders take codes the f64 decoder refuses;
  * the restatement tests/ldpc_llr_oracle.py agrees with the project's existing yardstick, oracle.ldpc_sum_product, on the decisions
    of every word both finish, and the layered schedule needs no more iterations than the flooding one."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import ldpc_llr_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANION = os.path.join(ROOT, 'include', 'fgnn_hip_ldpc_llr.h')
NEW = ('fgnn_ldpc_decode_llr', 'fgnn_ldpc_decode_llr_lds_bytes')
EINVAL = -1                                    # FGNN_EINVAL


def test_companion_header_is_parsed_bound_and_built():
    from fgnn_amd import _hip
    text = open(COMPANION).read()
    assert '#include "fgnn_hip.h"' in text and 'extern "C"' in text
    sig = _hip.signatures(text)
    assert tuple(sig) == NEW == _hip.LDPC_LLR
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
    assert [n for n, _ in sig[NEW[0]][1]] == ['llr', 'llr_sb', 'col_ptr', 'row_ptr', 'row_edge', 'row_var', 'layer_ptr', 'layer_chk',
                                              'n_layers', 'B', 'N', 'M', 'E', 'algorithm', 'max_iter', 'alpha', 'beta', 'x', 'post',
                                              'viol', 'iters', 'stream']
    args = dict(sig[NEW[0]][1])
    assert args['alpha'] is ctypes.c_float and args['beta'] is ctypes.c_float and args['B'] is ctypes.c_int64
    assert args['llr_sb'] is ctypes.c_int64 and args['llr'] is _hip.DevicePointer and args['stream'] is _hip.DevicePointer
    assert [n for n, _ in sig[NEW[1]][1]] == ['N', 'M', 'E']
    assert text.count('No counterpart in the reference') == 2        # each prototype says why it exists


def test_library_footprint_and_validation_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    q = lambda n, m, e: int(_hip.invoke('fgnn_ldpc_decode_llr_lds_bytes', n, m, e))
    # per word: f32 R [E], T [N], prior [N]; the packed row table [E]; 16-bit row_ptr, col_ptr, layer_chk, layer_ptr; 4 wave counts
    want = lambda n, m, e: (4 * (2 * e + 2 * n) + (2 * ((m + 1) + (n + 1) + m + (m + 1)) + 3) // 4 * 4 + 16 + 15) // 16 * 16
    for n, m, e in ((96, 48, 288), (12, 6, 36), (1024, 512, 4096), (1024, 1024, 16384), (1, 1, 1)):
        assert q(n, m, e) == want(n, m, e), (n, m, e)
    assert q(96, 48, 288) < 4096 < 140 * 1024 < q(1024, 1024, 16384) <= 160 * 1024         # sized by the code, not by the maxima
    sizes = [q(1024, 1024, e) for e in range(1024, 16385, 512)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))                                     # grows with E
    for n, m, e in ((1025, 48, 288), (0, 48, 288), (96, 1025, 288), (96, 0, 288), (96, 48, 0), (96, 48, -1), (1024, 1024, 16385),
                    (96, 48, 16 * 48 + 1), (8, 48, 16 * 8 + 1)):
        assert q(n, m, e) == -1, (n, m, e)
    assert b'variables' in (q(1025, 48, 288), L.fgnn_last_error())[1]
    assert b'checks' in (q(96, 1025, 288), L.fgnn_last_error())[1]
    assert b'edges' in (q(96, 48, 769), L.fgnn_last_error())[1]

    one = ctypes.c_void_p(16)                      # a non-NULL pointer that is never dereferenced on these paths
    def dec(llr=one, sb=96, tab=one, lp=one, lc=one, nl=0, B=4, n=96, m=48, e=288, alg=0, it=50, alpha=0.8125, beta=0.5, x=one,
            viol=one, iters=one):
        return _hip.invoke('fgnn_ldpc_decode_llr', llr, sb, tab, tab, tab, tab, lp, lc, nl, B, n, m, e, alg, it, alpha, beta, x, None,
                           viol, iters, None)
    assert dec(n=1025) == _hip.EUNSUPPORTED and dec(m=1025) == _hip.EUNSUPPORTED and dec(e=16 * 48 + 1) == _hip.EUNSUPPORTED
    assert dec(n=0) == _hip.EUNSUPPORTED and dec(e=0) == _hip.EUNSUPPORTED
    assert dec(alg=3) == _hip.EUNSUPPORTED and dec(alg=-1) == _hip.EUNSUPPORTED and b'algorithm' in L.fgnn_last_error()
    assert dec(it=0) == EINVAL and b'max_iter' in L.fgnn_last_error()
    for v in (-0.5, float('nan'), float('inf')):
        assert dec(alpha=v) == EINVAL and b'alpha' in L.fgnn_last_error()
        assert dec(beta=v) == EINVAL and b'beta' in L.fgnn_last_error()
    assert dec(sb=-1) == EINVAL and b'stride' in L.fgnn_last_error()
    assert dec(B=-1) == EINVAL and dec(B=2 ** 31) == EINVAL and b'batch' in L.fgnn_last_error()
    assert dec(nl=-1) == EINVAL and dec(nl=49) == EINVAL and b'n_layers' in L.fgnn_last_error()
    assert dec(llr=None) == EINVAL and dec(tab=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert dec(x=None) == EINVAL and dec(viol=None) == EINVAL and dec(iters=None) == EINVAL
    assert dec(nl=5, lp=None) == EINVAL and dec(nl=5, lc=None) == EINVAL and b'layer' in L.fgnn_last_error()
    assert dec(llr=None, tab=None, lp=None, lc=None, x=None, viol=None, iters=None, B=0) == 0      # empty batch: nothing to do
    assert dec(llr=None, tab=None, lp=None, lc=None, x=None, viol=None, iters=None, B=0, nl=5) == 0
    assert dec(B=0, n=1025) == _hip.EUNSUPPORTED and dec(B=0, it=0) == EINVAL                      # sizes are checked even then


def test_layers_partition_the_checks():
    from fgnn_amd.ldpc_code import LdpcCode
    for code in (LdpcCode.builtin(), LdpcCode.gallager(24, 3, 6, 0), LdpcCode.gallager(32, 16, 16, 3), LdpcCode.gallager(384, 3, 6, 1)):
        lp, lc = code.layers()
        assert code.layers()[0] is lp and lp.dtype == np.int32 and lc.dtype == np.int32                # memoised
        assert lp[0] == 0 and lp[-1] == code.n_chk and (np.diff(lp) > 0).all()
        assert sorted(lc) == list(range(code.n_chk))
        rows = [set(np.nonzero((code.nlist == m).any(1))[0]) for m in range(code.n_chk)]
        for k in range(len(lp) - 1):
            members = lc[lp[k]:lp[k + 1]]
            assert list(members) == sorted(members)
            seen = set()
            for m in members:
                assert not seen & rows[m]
                seen |= rows[m]
            for m in lc[lp[k + 1]:]:                                       # greedy: a later check did not fit this layer when it came
                assert any(rows[m] & rows[o] for o in members if o < m)
    g = LdpcCode.gallager(24, 3, 6, 0)                                     # the bands: 3 layers of 4 consecutive checks
    lp, lc = g.layers()
    assert list(lp) == [0, 4, 8, 12] and list(lc) == list(range(12))
    with pytest.raises(ValueError):
        lp[0] = 1


def test_require_llr_decoder():
    from fgnn_amd.ldpc_code import LdpcCode
    big = LdpcCode.gallager(1024, 4, 8, 2)
    assert big.require_llr_decoder() is big
    with pytest.raises(ValueError, match='edges'):
        big.require_decoder()
    wide = LdpcCode.gallager(34, 17, 17, 0)
    with pytest.raises(ValueError, match='degree 17'):
        wide.require_llr_decoder()
    tall = LdpcCode.gallager(1024, 9, 8, 0)                                # M = 1152 checks
    with pytest.raises(ValueError, match='M = 1152 checks'):
        tall.require_llr_decoder()
    import fgnn_amd.ldpc_code as C
    assert 'require_llr_decoder' in C.__doc__ and (C.LLR_MAXV, C.LLR_MAXD) == (1024, 16)


# decoder specs -> parse_decoder's (canonical spec, kind, arguments), and specs it refuses: test_ldpc_nms.py and test_ldpc_osd.py hold
# the parser to the same table
PARSED = (
    ('mackay', 'mackay', 'mackay', {'loops': 100}),
    ('mackay:iters=20', 'mackay:iters=20', 'mackay', {'loops': 20}),
    ('min-sum', 'min-sum:flooding', 'llr', dict(algorithm='min-sum', schedule='flooding', max_iter=50, alpha=0.8125, beta=0.5)),
    ('min-sum:layered', 'min-sum:layered', 'llr', dict(algorithm='min-sum', schedule='layered', max_iter=50, alpha=0.8125, beta=0.5)),
    ('min-sum:alpha=0.75', 'min-sum:flooding:alpha=0.75', 'llr',
     dict(algorithm='min-sum', schedule='flooding', max_iter=50, alpha=0.75, beta=0.5)),
    ('offset-min-sum:layered:beta=0.25', 'offset-min-sum:layered:beta=0.25', 'llr',
     dict(algorithm='offset-min-sum', schedule='layered', max_iter=50, alpha=0.8125, beta=0.25)),
    ('sum-product:flooding:iters=100', 'sum-product:flooding:iters=100', 'llr',
     dict(algorithm='sum-product', schedule='flooding', max_iter=100, alpha=0.8125, beta=0.5)),
    ('sum-product:layered:iters=50', 'sum-product:layered', 'llr',
     dict(algorithm='sum-product', schedule='layered', max_iter=50, alpha=0.8125, beta=0.5)))
JUNK = ('', None, 7, 'max-sum', 'min-sum:', 'min-sum:zigzag', 'min-sum:layered:flooding', 'min-sum:iters=0', 'min-sum:iters=x',
        'min-sum:iters=2:iters=3', 'min-sum:alpha=-1', 'min-sum:alpha=nan', 'min-sum:alpha=inf', 'min-sum:beta=0.5',
        'offset-min-sum:alpha=0.5', 'sum-product:alpha=0.5', 'min-sum:iters=3:layered', 'mackay:layered', 'mackay:alpha=1',
        'min-sum:gamma=1', 'min-sum:iters')


def test_parse_decoder_round_trips_and_refuses_junk():
    from fgnn_amd.ldpc_eval import parse_decoder
    for spec, canon, kind, kw in PARSED:
        got = parse_decoder(spec)
        assert got == (canon, kind, kw), spec
        assert parse_decoder(canon) == got                                  # the canonical spec parses to itself
    for junk in JUNK:
        with pytest.raises(ValueError):
            parse_decoder(junk)


def test_check_decode_llr_args():
    import torch
    from fgnn_amd.ldpc_decoders import check_decode_llr_args
    llr = torch.zeros(5, 96)
    ok = dict(llr=llr, n_var=96, algorithm='min-sum', schedule='flooding', max_iter=50, alpha=0.8125, beta=0.5)
    assert check_decode_llr_args(**ok) == (5, 0)
    assert check_decode_llr_args(**dict(ok, algorithm='offset-min-sum'))[1] == 1
    assert check_decode_llr_args(**dict(ok, algorithm='sum-product', schedule='layered', llr=torch.zeros(0, 96, dtype=torch.float64))) == (0, 2)
    for kw, what in (({'algorithm': 'max-sum'}, 'algorithm'), ({'algorithm': 0}, 'algorithm'), ({'schedule': 'serial'}, 'schedule'),
                     ({'max_iter': 0}, 'max_iter'), ({'max_iter': 2.5}, 'max_iter'), ({'max_iter': True}, 'max_iter'),
                     ({'max_iter': 2 ** 31}, 'max_iter'), ({'alpha': -0.1}, 'alpha'), ({'alpha': float('nan')}, 'alpha'),
                     ({'alpha': float('inf')}, 'alpha'), ({'beta': -1}, 'beta'), ({'beta': 1e39}, 'beta'),
                     ({'llr': torch.zeros(5, 95)}, 'llr'), ({'llr': torch.zeros(96)}, 'llr'), ({'llr': np.zeros((5, 96))}, 'llr'),
                     ({'llr': torch.zeros(5, 96, dtype=torch.int32)}, 'floating')):
        with pytest.raises(ValueError, match=what):
            check_decode_llr_args(**dict(ok, **kw))


def test_decode_llr_needs_a_device_and_validates_first():
    import torch
    from fgnn_amd.datapath import LdpcDataPath
    with pytest.raises(RuntimeError):
        LdpcDataPath('cpu')
    path = LdpcDataPath.__new__(LdpcDataPath)                                # host side only: no device is touched
    path.N, path.device = 96, torch.device('cuda:0')
    with pytest.raises(ValueError, match='algorithm'):
        path.decode_llr(torch.zeros(2, 96), algorithm='bp')
    with pytest.raises(ValueError, match='llr'):
        path.decode_llr(torch.zeros(2, 97))
    from fgnn_amd.ldpc_eval import evaluate
    with pytest.raises(ValueError, match='decoder'):
        evaluate(torch.nn.Linear(1, 1), {}, baseline=['min-sum:diagonal'])


@functools.lru_cache(maxsize=None)
def words():
    """The built-in code and 256 received words of the all-zero codeword at 4 dB, no burst, from a fixed numpy seed."""
    from fgnn_amd.ldpc_code import LdpcCode
    code = LdpcCode.builtin()
    rng = np.random.RandomState(20261019)
    gcx = 10.0 ** (4.0 / 20.0)
    y = (-gcx + rng.standard_normal((256, 96))).astype(np.float32)
    llr = (np.float32(-2.0 * gcx) * y).astype(np.float32)
    return code, LO.tables(code.nlist, code.n_chk), y, llr


def test_restatement_against_the_reference_sum_product():
    """The f64 flooding sum-product restatement (100 iterations) against oracle.ldpc_sum_product (MacKay's probability-domain decoder,
    100 loops): the same decisions on every word both finish.  Words exactly one of the two finishes: 0 of 256 (both finish all 256
    at this SNR) — measured on the CPU, deterministic, pinned."""
    import fgnn_oracle as O
    code, tabs, y, llr = words()
    r = LO.decode(llr, tabs, None, 'sum-product', 100, dtype=np.float64)
    bias = O.ldpc_bit_prior(y, np.full(256, 4.0))
    both = one = 0
    for b in range(256):
        x, _, viol, _ = O.ldpc_sum_product(code.nlist, code.n_chk, bias[b], 100)
        mine, theirs = r['viol'][b] == 0, viol == 0
        if mine and theirs:
            both += 1
            assert np.array_equal(x, r['x'][b]), b
        else:
            one += int(mine != theirs)
    print('both finish %d, exactly one finishes %d' % (both, one))
    assert one == 0 and both == 256


def test_layered_needs_no_more_iterations_than_flooding():
    code, tabs, _, llr = words()
    flood = LO.decode(llr, tabs, None, 'min-sum', 50)
    layered = LO.decode(llr, tabs, code.layers(), 'min-sum', 50)
    print('iterations in total: flooding %d, layered %d' % (flood['iters'].sum(), layered['iters'].sum()))
    assert layered['iters'].sum() <= flood['iters'].sum()
    assert (flood['viol'] == 0).all() and (layered['viol'] == 0).all() and not flood['x'].any() and not layered['x'].any()


def test_restatement_properties():
    """f32 and f64 agree closely after one iteration; a degree-1 check sends 0; margin is the smallest |T| seen."""
    code, tabs, _, llr = words()
    a = LO.decode(llr[:16], tabs, None, 'sum-product', 1)
    b = LO.decode(llr[:16], tabs, None, 'sum-product', 1, dtype=np.float64)
    assert a['post'].dtype == np.float32 and b['post'].dtype == np.float64
    # one iteration from LLRs up to about 15: a message m = 2 atanh(p) moves by 2 ulp(p) / (1 - p^2) ~ 2^-24 e^m / 2, below 1e-3 for m <= 10
    assert np.abs(a['post'] - b['post']).max() <= 1e-3 and np.array_equal(a['x'], b['x'])
    assert np.array_equal(b['margin'], np.abs(b['post']).min(1))
    tabs1 = LO.tables(np.array([[0, 1], [0, -1]]), 2)                        # check 1 has one variable
    tabs0 = LO.tables(np.array([[0], [0]]), 1)                               # the same code without it
    for alg in LO.ALGORITHMS:
        for layers in (None, (np.array([0, 2]), np.array([0, 1]))):
            r = LO.decode(np.array([[1.5, -0.5]], np.float32), tabs1, layers, alg, 1)
            r0 = LO.decode(np.array([[1.5, -0.5]], np.float32), tabs0, None if layers is None else (np.array([0, 1]), np.array([0])), alg, 1)
            assert np.array_equal(r['post'], r0['post'])
    r = LO.decode(np.array([[1.5, -0.5]], np.float32), tabs1, None, 'min-sum', 1)
    assert list(r['post'][0]) == [1.5 - 0.8125 * 0.5, -0.5 + 0.8125 * 1.5]
