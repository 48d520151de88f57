"""CPU: ordered-statistics reprocessing's checker and host side (csrc/ldpc_osd.hip, include/fgnn_hip_ldpc_osd.h,
LdpcDataPath.decode_osd, ldpc_eval.parse_decoder's ``osd=`` / ``span=`` options) and the restatement tests/ldpc_osd_oracle.py.

  * the companion header binds beside the others, whose interface is what it was;
  * every refusal of both entry points happens before any launch, so it is testable without a device;
  * the restatement's own properties on the GPU test's inputs: the cost never rises with the order or the span, metric=None is
    metric=rel, pass-through words are untouched, equal reliabilities resolve by index;
  * statistical sanity of the definition, on the restatement alone: the built-in code at 2.5 dB, 400 words of the all-zero codeword
    (test_ldpc_llr_gpu.received's construction, seed 20261021), layered min-sum with 20 iterations.  Word errors over the 48 message
    bits: plain 29, osd=1 9, osd=2 (span 64) 7 — measured on the CPU, deterministic; the test requires only that reprocessing does
    not add word errors."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import ldpc_llr_oracle as LO
import ldpc_osd_oracle as OO
import test_ldpc_osd_gpu as G
from test_ldpc_llr import JUNK, PARSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANION = os.path.join(ROOT, 'include', 'fgnn_hip_ldpc_osd.h')
NEW = ('fgnn_ldpc_osd', 'fgnn_ldpc_osd_lds_bytes')
EINVAL = -1                                    # FGNN_EINVAL


def test_companion_header_is_parsed_bound_and_built():
    from fgnn_amd import _hip
    text = open(COMPANION).read()
    assert '#include "fgnn_hip.h"' in text and 'extern "C"' in text
    sig = _hip.signatures(text)
    assert tuple(sig) == NEW == _hip.LDPC_OSD
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
    assert [n for n, _ in sig[NEW[0]][1]] == ['rel', 'rel_sb', 'metric', 'metric_sb', 'viol', 'row_ptr', 'row_var', 'B', 'N', 'M', 'E',
                                              'order', 'span', 'x', 'cost', 'pattern', 'stream']
    args = dict(sig[NEW[0]][1])
    assert args['B'] is ctypes.c_int64 and args['rel_sb'] is ctypes.c_int64 and args['metric_sb'] is ctypes.c_int64
    assert args['order'] is ctypes.c_int32 and args['span'] is ctypes.c_int32
    assert args['rel'] is _hip.DevicePointer and args['viol'] is _hip.DevicePointer and args['stream'] is _hip.DevicePointer
    assert [n for n, _ in sig[NEW[1]][1]] == ['N', 'M']
    assert text.count('No counterpart in the reference') == 2        # each prototype says why it exists
    for other in ('LDPC_LLR', 'LDPC_NMS', 'LDPC_CODE', 'LDPC_TRAIN', 'PGM_BP', 'WGRAD'):          # the others are bound as before
        assert all(_hip.COMPANIONS[n][2] != 'fgnn_hip_ldpc_osd.h' for n in getattr(_hip, other))


def test_library_footprint_and_validation_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    q = lambda n, m: int(_hip.invoke('fgnn_ldpc_osd_lds_bytes', n, m))
    # per word: the matrix [M][RW] (RW = ceil((N + 1) / 32) made odd), keys and signed weights [N], 32 scratch words; 16-bit order and
    # non-pivot list [N], pivot columns and rows [M]; the bits as bytes [N]
    want = lambda n, m: (4 * (m * (((n + 32) // 32) | 1) + 2 * n + 32) + 2 * (2 * n + 2 * m) + n + 15) // 16 * 16
    for n, m in ((96, 48), (12, 6), (63, 27), (64, 24), (1024, 512), (1024, 1024), (1, 1), (20, 70)):
        assert q(n, m) == want(n, m), (n, m)
    assert q(96, 48) < 4096 and 132 * 1024 < q(1024, 1024) < 160 * 1024
    for n, m in ((1025, 48), (0, 48), (-1, 48), (96, 1025), (96, 0)):
        assert q(n, m) == -1, (n, m)
    assert b'variables' in (q(1025, 48), L.fgnn_last_error())[1]
    assert b'checks' in (q(96, 1025), L.fgnn_last_error())[1]

    one = ctypes.c_void_p(16)                      # a non-NULL pointer that is never dereferenced on these paths
    def osd(rel=one, sb=96, metric=one, msb=96, viol=one, tab=one, B=4, n=96, m=48, e=288, order=1, span=96, x=one, cost=one, pattern=one):
        return _hip.invoke('fgnn_ldpc_osd', rel, sb, metric, msb, viol, tab, tab, B, n, m, e, order, span, x, cost, pattern, None)
    assert osd(n=1025) == _hip.EUNSUPPORTED and b'variables' in L.fgnn_last_error()
    assert osd(n=0) == _hip.EUNSUPPORTED and osd(m=1025) == _hip.EUNSUPPORTED and osd(m=0) == _hip.EUNSUPPORTED
    assert osd(e=0) == _hip.EUNSUPPORTED and osd(e=16 * 48 + 1) == _hip.EUNSUPPORTED and b'edges' in L.fgnn_last_error()
    assert osd(order=3) == _hip.EUNSUPPORTED and osd(order=-1) == _hip.EUNSUPPORTED and b'order' in L.fgnn_last_error()
    assert osd(order=2, span=257) == _hip.EUNSUPPORTED and b'span' in L.fgnn_last_error()
    assert osd(span=0) == EINVAL and osd(span=-3) == EINVAL and osd(order=0, span=0) == EINVAL and b'span' in L.fgnn_last_error()
    assert osd(sb=-1) == EINVAL and osd(msb=-1) == EINVAL and b'stride' in L.fgnn_last_error()
    assert osd(B=-1) == EINVAL and osd(B=2 ** 31) == EINVAL and b'batch' in L.fgnn_last_error()
    assert osd(rel=None) == EINVAL and osd(tab=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert osd(x=None) == EINVAL and osd(cost=None) == EINVAL and osd(pattern=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert osd(rel=None, metric=None, viol=None, tab=None, x=None, cost=None, pattern=None, B=0) == 0      # empty batch: nothing to do
    assert osd(B=0, n=1025) == _hip.EUNSUPPORTED and osd(B=0, span=0) == EINVAL                            # sizes are checked even then
    assert osd(B=0, order=2, span=257) == _hip.EUNSUPPORTED and osd(B=0, order=1, span=2000) == 0         # (the span is clipped)


def test_check_decode_osd_args():
    import torch
    from fgnn_amd.ldpc_decoders import check_decode_osd_args
    rel = torch.zeros(5, 96)
    ok = dict(rel=rel, metric=None, viol=None, n_var=96, order=1, span=None)
    assert check_decode_osd_args(**ok) == (5, 96)                                          # the default spans
    assert check_decode_osd_args(**dict(ok, order=0)) == (5, 96) and check_decode_osd_args(**dict(ok, order=2)) == (5, 64)
    assert check_decode_osd_args(**dict(ok, order=2, span=256, metric=torch.zeros(5, 96, dtype=torch.float64),
                                        viol=torch.zeros(5, dtype=torch.int32))) == (5, 256)
    assert check_decode_osd_args(**dict(ok, rel=torch.zeros(0, 96), span=2000)) == (0, 2000)
    for kw, what in (({'order': 3}, 'order'), ({'order': -1}, 'order'), ({'order': 1.0}, 'order'), ({'order': True}, 'order'),
                     ({'order': '1'}, 'order'), ({'span': 0}, 'span'), ({'span': 2.5}, 'span'), ({'span': True}, 'span'),
                     ({'span': 2 ** 31}, 'span'), ({'order': 2, 'span': 257}, 'span'),
                     ({'rel': torch.zeros(5, 95)}, 'rel'), ({'rel': torch.zeros(96)}, 'rel'), ({'rel': np.zeros((5, 96))}, 'rel'),
                     ({'rel': torch.zeros(5, 96, dtype=torch.int32)}, 'floating'), ({'metric': torch.zeros(5, 95)}, 'metric'),
                     ({'metric': torch.zeros(4, 96)}, 'metric'), ({'metric': torch.zeros(5, 96, dtype=torch.int64)}, 'floating'),
                     ({'viol': torch.zeros(4, dtype=torch.int32)}, 'viol'), ({'viol': torch.zeros(5, dtype=torch.int64)}, 'viol'),
                     ({'viol': np.zeros(5, np.int32)}, 'viol'), ({'viol': torch.zeros(5, 1, dtype=torch.int32)}, 'viol')):
        with pytest.raises(ValueError, match=what):
            check_decode_osd_args(**dict(ok, **kw))


def test_decode_osd_validates_before_the_device():
    import torch
    from fgnn_amd.datapath import LdpcDataPath
    path = LdpcDataPath.__new__(LdpcDataPath)                                # host side only: no device is touched
    path.N, path.device = 96, torch.device('cuda:0')
    with pytest.raises(ValueError, match='order'):
        path.decode_osd(torch.zeros(2, 96), order=3)
    with pytest.raises(ValueError, match='rel'):
        path.decode_osd(torch.zeros(2, 97))
    with pytest.raises(ValueError, match='span'):
        path.decode_osd(torch.zeros(2, 96), order=2, span=300)
    from fgnn_amd.ldpc_eval import evaluate
    with pytest.raises(ValueError, match='decoder'):
        evaluate(torch.nn.Linear(1, 1), {}, baseline=['min-sum:layered:osd=3'])


def test_parse_decoder_takes_osd_and_span():
    from fgnn_amd.ldpc_eval import parse_decoder
    ms = dict(algorithm='min-sum', schedule='layered', max_iter=50, alpha=0.8125, beta=0.5)
    for spec, canon, kw in (
            ('min-sum:layered:osd=1', 'min-sum:layered:osd=1', dict(ms, osd=1)),
            ('min-sum:layered:osd=2:span=24', 'min-sum:layered:osd=2:span=24', dict(ms, osd=2, span=24)),
            ('min-sum:layered:iters=20:osd=2:span=256', 'min-sum:layered:iters=20:osd=2:span=256', dict(ms, max_iter=20, osd=2, span=256)),
            ('min-sum:layered:span=700:osd=1', 'min-sum:layered:osd=1:span=700', dict(ms, osd=1, span=700)),
            ('sum-product:osd=0', 'sum-product:flooding:osd=0', dict(ms, algorithm='sum-product', schedule='flooding', osd=0)),
            ('offset-min-sum:osd=1:beta=0.25', 'offset-min-sum:flooding:beta=0.25:osd=1',
             dict(ms, algorithm='offset-min-sum', schedule='flooding', beta=0.25, osd=1))):
        got = parse_decoder(spec)
        assert got == (canon, 'llr', kw), spec
        assert parse_decoder(canon) == got                                  # the canonical spec parses to itself
    # the table of test_ldpc_llr.py: identical triples, no 'osd' and no 'span' among the arguments
    for spec, canon, kind, kw in PARSED:
        assert parse_decoder(spec) == (canon, kind, kw), spec
    for junk in ('min-sum:osd=3', 'min-sum:osd=-1', 'min-sum:span=4', 'min-sum:osd=0:span=4', 'min-sum:osd=2:span=257', 'mackay:osd=1',
                 'min-sum:osd=1:osd=1', 'min-sum:osd=1:span=0', 'min-sum:span=0', 'min-sum:osd', 'min-sum:osd=x', 'min-sum:osd=1.5',
                 'min-sum:osd=1:span=2:span=2', 'min-sum:osd=1:layered', 'mackay:span=4', 'learned-min-sum', 'min-sum:osd=1:span=-1',
                 # the junk of test_ldpc_llr.py stays junk
                 *JUNK):
        with pytest.raises(ValueError):
            parse_decoder(junk)
    assert parse_decoder('learned-min-sum:a:osd=1')[2] == {'path': 'a:osd=1'}           # (a learned spec: all of it is the path)


@pytest.mark.parametrize('name', ('g12', 'g33', 'builtin', 'g32', 'g384'))
def test_cost_never_rises_with_order_or_span(name):
    nf = G.free_positions(name)
    cost = {s: G.restated(name, *s)[1].astype(np.int64) for s in G.settings(name)}
    assert np.array_equal(cost[(0, 1)], cost[(0, nf + 5)])                               # order 0 has no span
    for order in (1, 2):
        spans = sorted(s for o, s in cost if o == order)
        assert (cost[(order, spans[0])] <= cost[(0, 1)]).all()
        for a, b in zip(spans, spans[1:]):
            assert (cost[(order, b)] <= cost[(order, a)]).all(), (order, a, b)
    for span in sorted({s for o, s in cost if o == 1} & {s for o, s in cost if o == 2}):
        assert (cost[(2, span)] <= cost[(1, span)]).all()
    assert np.array_equal(cost[(1, nf)], cost[(1, nf + 5)])                              # the span is clipped at N - rank
    assert (cost[(1, nf)] < cost[(0, 1)]).any()                                          # (and the inputs make the order matter)
    for order, span in cost:                                                             # a longer list keeps the earlier indices
        pattern = G.restated(name, order, span)[2]
        assert (pattern >= 0).all() and (pattern <= span + span * (span - 1) // 2).all()
        assert order > 0 or not pattern.any()


def test_metric_none_pass_through_and_ties():
    code, _, H, llr, bp = G.case('builtin')
    a = OO.reprocess(bp['post'], None, None, H, 1, 96)
    b = OO.reprocess(bp['post'], bp['post'], None, H, 1, 96)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))                               # metric=None is metric=rel
    viol = bp['viol'].astype(np.int32)
    x, cost, pattern = OO.reprocess(bp['post'], llr, viol, H, 2, 24)
    through = viol == 0
    assert through.any() and (~through).any()
    h = (bp['post'] < 0).astype(np.uint8)
    assert np.array_equal(x[through], h[through]) and (pattern[through] == -1).all() and (pattern[~through] >= 0).all()
    assert np.array_equal(cost[through], (OO.quantise(llr) * (h ^ (llr < 0))).sum(1)[through])
    assert np.array_equal(x[through], bp['x'][through]) and not (H.astype(np.int64) @ x.T.astype(np.int64) % 2).any()
    full = OO.reprocess(bp['post'], llr, None, H, 2, 24, G.eliminated('builtin'))
    assert all(np.array_equal(u[~through], v[~through]) for u, v in zip((x, cost, pattern), full))
    # equal reliabilities: the order is the index order, so the pivots are the greedy independent columns from the left and the
    # non-pivot list is the other columns, ascending
    flat = np.full((1, 96), 0.5, np.float32)
    st = OO.eliminate(flat[0], llr[0], H)
    assert list(st['order']) == list(range(96))
    assert list(st['free']) == sorted(st['free']) and list(st['piv']) == sorted(st['piv'])
    rank, piv = 0, []
    for c in range(96):                                                                  # (rank by rank, the slow way)
        r = _rank(H[:, piv + [c]])
        if r > rank:
            rank, piv = r, piv + [c]
    assert piv == list(st['piv'])
    # ... and among equal costs the lowest index wins: a metric of zeros makes every candidate cost 0
    x, cost, pattern = OO.reprocess(bp['post'][:8], np.zeros((8, 96), np.float32), None, H, 2, 24)
    assert not cost.any() and not pattern.any()


def _rank(A):
    """The rank over GF(2), by row echelon form."""
    A, r = A.astype(np.uint8) % 2, 0
    for c in range(A.shape[1]):
        rows = r + np.nonzero(A[r:, c])[0]
        if rows.size:
            A[[r, rows[0]]] = A[[rows[0], r]]
            A[rows[1:]] ^= A[r]
            r += 1
    return r


@functools.lru_cache(maxsize=None)
def sanity():
    from fgnn_amd.ldpc_code import LdpcCode
    code = LdpcCode.builtin()
    tabs = LO.tables(code.nlist, code.n_chk)
    H = OO.dense(tabs[1], tabs[3], 96)
    llr = G.received(code, 20261021, (2.5, 2.5), 400)
    bp = LO.decode(llr, tabs, code.layers(), 'min-sum', 20)
    sts = OO.states(bp['post'], llr, H, bp['viol'])
    errors = lambda x: int(x[:, :code.K].any(1).sum())                                    # the all-zero codeword was sent
    return (errors(bp['x']), errors(OO.reprocess(bp['post'], llr, bp['viol'], H, 1, 96, sts)[0]),
            errors(OO.reprocess(bp['post'], llr, bp['viol'], H, 2, 64, sts)[0]))


def test_reprocessing_adds_no_word_errors():
    plain, osd1, osd2 = sanity()
    print('word errors of 400 at 2.5 dB: min-sum:layered:iters=20 %d, osd=1 %d, osd=2 %d' % (plain, osd1, osd2))
    assert osd1 <= plain and osd2 <= plain
