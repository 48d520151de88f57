"""CPU: the learned min-sum LDPC decoder's checker and host side (csrc/ldpc_nms.hip, include/fgnn_hip_ldpc_nms.h, fgnn_amd/ldpc_nms.py,
ldpc_eval.parse_decoder), and the inputs tests/test_ldpc_nms_gpu.py shares with this file.

  * the companion header binds beside the main one, whose interface is what it was;
  * argument validation of the entry points happens before any launch, so it is testable without a device;
  * the f32 restatement tests/ldpc_nms_oracle.py with constant weights is the existing restatement tests/ldpc_llr_oracle.py bit for
    bit (min-sum with beta = 0, offset min-sum with alpha = 1), which pins the new one to the old;
  * its explicit backward recursion equals torch autograd's over the float64 forward, and finite differences;
  * the inputs of the GPU comparison: at most 5 % of the words have a record that differs between the restatement's two precisions, and
    the restatement's own f32 error is what test_ldpc_nms_gpu.py says it is.

Inputs of the GPU file (``words``, ``weights``, ``g_totals``): the received words of tests/test_ldpc_llr_gpu.py (``case``: B = 67 at its
``SNR_DB``; for g1024 the five words 0, 16, 32, 48, 64 of them, which span its SNR range), alpha in [0.3, 1.2] and beta in [0, 0.4]
drawn per weight from a fixed seed, g_totals N(0, 1) from a fixed seed."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import ldpc_llr_oracle as LO
import ldpc_nms_oracle as NO
import test_ldpc_llr_gpu as LG
from test_ldpc_llr import JUNK, PARSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANION = os.path.join(ROOT, 'include', 'fgnn_hip_ldpc_nms.h')
NEW = ('fgnn_ldpc_nms_forward', 'fgnn_ldpc_nms_backward', 'fgnn_ldpc_nms_record_bytes', 'fgnn_ldpc_nms_backward_workspace_bytes',
       'fgnn_ldpc_nms_lds_bytes', 'fgnn_ldpc_nms_backward_workgroups')
EINVAL = -1                                    # FGNN_EINVAL

CODES = ('g12', 'builtin', 'g32', 'g1024')
N_ITER = {'g12': 5, 'builtin': 5, 'g32': 5, 'g1024': 3}
SHARES = NO.SHARES
# d per output tensor: the largest |g_f32 - g_f64| / max |g_f64| between the restatement's own two precisions (``NO.backward`` on
# ``NO.forward`` in float32 and in float64) over every (code, share) below, on the words whose two records agree; measured on the
# CPU by ``restatement_error`` (python tests/test_ldpc_nms.py prints it).  The GPU bound is 4 d, as SP_BOUND is formed.
D = {'g_alpha': 2.967e-07, 'g_beta': 3.674e-07, 'g_llr': 1.750e-07}      # measured; no word is left out in any case
LEFT_OUT_CAP = 0.05


def words(name):
    llr = LG.case(name)[3]
    return llr[::16][:5] if name == 'g1024' else llr


def tabs(name):
    return LG.case(name)[1]


@functools.lru_cache(maxsize=None)
def weights(name, share, n_iter=None):
    """(alpha, beta) [n_iter, W] f32: alpha in [0.3, 1.2], beta in [0, 0.4], one draw per weight."""
    n_iter = N_ITER[name] if n_iter is None else n_iter
    rng = np.random.RandomState(3000 + 3 * CODES.index(name) + SHARES.index(share))
    W = NO.weight_count(share, tabs(name))
    alpha, beta = rng.uniform(0.3, 1.2, (n_iter, W)).astype(np.float32), rng.uniform(0.0, 0.4, (n_iter, W)).astype(np.float32)
    alpha.setflags(write=False)
    beta.setflags(write=False)
    return alpha, beta


@functools.lru_cache(maxsize=None)
def g_totals(name):
    g = np.random.RandomState(4000 + CODES.index(name)).standard_normal((N_ITER[name],) + words(name).shape).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def restated(name, share, dtype='float32'):
    """The restatement's train-mode forward on ``words(name)`` with ``weights(name, share)``: computed once, shared, never written."""
    alpha, beta = weights(name, share)
    return NO.forward(words(name), tabs(name), alpha, beta, share, N_ITER[name], np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def kept(name, share):
    """[B] bool: the words whose f32 and f64 records agree in every field (a flipped minimum is another function, not an error)."""
    return NO.same_record(restated(name, share), restated(name, share, 'float64'))


@functools.lru_cache(maxsize=None)
def restated_backward(name, share, dtype='float64'):
    """(g_alpha, g_beta, g_llr) of the explicit recursion on the kept words."""
    return NO.backward(restated(name, share, dtype), g_totals(name), kept(name, share))


def relative_error(got, want):
    """The largest |got - want| / max |want|, per tensor."""
    return [float(np.abs(np.asarray(g, np.float64) - w).max() / np.abs(w).max()) for g, w in zip(got, want)]


def restatement_error():
    """({tensor: d}, the largest fraction of words left out in any case)."""
    d, out = dict.fromkeys(D, 0.0), 0.0
    for name in CODES:
        for share in SHARES:
            err = relative_error(restated_backward(name, share, 'float32'), restated_backward(name, share))
            d = {k: max(d[k], e) for k, e in zip(D, err)}
            out = max(out, float((~kept(name, share)).mean()))
    return d, out


def test_companion_header_is_parsed_bound_and_built():
    from fgnn_amd import _hip
    text = open(COMPANION).read()
    assert '#include "fgnn_hip.h"' in text and 'extern "C"' in text
    sig = _hip.signatures(text)
    assert tuple(sig) == NEW == _hip.LDPC_NMS
    assert not set(NEW) & set(_hip.EXPORTS) and not set(NEW) & set(_hip.SIGNATURES) and _hip.ABI_VERSION == 15
    main = open(_hip.HEADER_PATH).read()
    assert not any(re.search(r'\b%s\b' % name, main) for name in NEW)
    L = _hip.lib()
    for name in NEW:
        fn = getattr(L, name)                                        # exported by the built library ...
        restype, params = sig[name]
        assert fn.restype is restype                                 # ... and bound with the parsed types
        assert list(fn.argtypes) == [t for _, t in params] and _hip.COMPANIONS[name][:2] == sig[name]
    assert [sig[n][0] for n in NEW] == [ctypes.c_int32] * 2 + [ctypes.c_int64] * 4
    assert [n for n, _ in sig[NEW[0]][1]] == ['llr', 'llr_sb', 'col_ptr', 'row_ptr', 'row_edge', 'row_var', 'alpha', 'beta', 'B', 'N', 'M',
                                              'E', 'n_iter', 'share', 'stop_early', 'x', 'post', 'viol', 'iters', 'totals', 'record',
                                              'record_bytes', 'stream']
    assert [n for n, _ in sig[NEW[1]][1]] == ['g_totals', 'llr', 'llr_sb', 'col_ptr', 'row_ptr', 'row_edge', 'row_var', 'alpha', 'beta',
                                              'record', 'record_bytes', 'B', 'N', 'M', 'E', 'n_iter', 'share', 'g_alpha', 'g_beta', 'g_llr',
                                              'workspace', 'workspace_bytes', 'stream']
    args = dict(sig[NEW[0]][1])
    assert args['alpha'] is _hip.DevicePointer and args['B'] is ctypes.c_int64 and args['record_bytes'] is ctypes.c_int64
    assert [n for n, _ in sig[NEW[2]][1]] == ['B', 'N', 'M', 'E', 'n_iter'] and [n for n, _ in sig[NEW[4]][1]] == ['N', 'M', 'E', 'backward']
    assert text.count('No counterpart in the reference') >= len(NEW)  # each prototype says why it exists


def test_size_queries_and_validation_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    lds = lambda n, m, e, bwd: int(_hip.invoke('fgnn_ldpc_nms_lds_bytes', n, m, e, bwd))
    # forward: f32 R [E], T [N], prior [N], the packed row table [E], 4 wave counts; 16-bit row_ptr, col_ptr.  backward: 8 wave sums.
    want = lambda n, m, e, bwd: (4 * (2 * e + 2 * n) + (32 if bwd else 16) + 15) // 16 * 16 + (2 * ((m + 1) + (n + 1)) + 15) // 16 * 16
    for n, m, e in ((96, 48, 288), (12, 6, 36), (1024, 512, 4096), (1024, 1024, 16384), (1, 1, 1)):
        assert lds(n, m, e, 0) == want(n, m, e, 0) and lds(n, m, e, 1) == want(n, m, e, 1), (n, m, e)
    assert lds(96, 48, 288, 0) < 4096 and lds(1024, 1024, 16384, 1) <= 160 * 1024          # sized by the code; within a CU's LDS
    # g1024's backward: state below 48 KiB, with the per-check partial (3 iterations) above it, with the per-edge one past the LDS budget
    assert lds(1024, 512, 4096, 1) < 48 * 1024 < lds(1024, 512, 4096, 1) + 8 * 3 * 512 <= 64 * 1024 < lds(1024, 512, 4096, 1) + 8 * 3 * 4096
    for n, m, e in ((1025, 48, 288), (0, 48, 288), (96, 1025, 288), (96, 0, 288), (96, 48, 0), (96, 48, -1), (1024, 1024, 16385),
                    (96, 48, 16 * 48 + 1), (8, 48, 16 * 8 + 1)):
        assert lds(n, m, e, 0) == -1 and lds(n, m, e, 1) == -1, (n, m, e)
    assert b'variables' in (lds(1025, 48, 288, 0), L.fgnn_last_error())[1]
    assert b'checks' in (lds(96, 1025, 288, 0), L.fgnn_last_error())[1]
    assert b'edges' in (lds(96, 48, 769, 0), L.fgnn_last_error())[1]
    rec = lambda *a: int(_hip.invoke('fgnn_ldpc_nms_record_bytes', *a))
    assert rec(67, 96, 48, 288, 5) == 67 * 5 * 48 * 12 and rec(0, 96, 48, 288, 5) == 0
    assert rec(2 ** 31 - 1, 1024, 1024, 16384, 64) == (2 ** 31 - 1) * 64 * 1024 * 12        # 64-bit
    assert rec(1, 1025, 48, 288, 5) == -1 and rec(1, 96, 48, 288, 0) == -1 and rec(1, 96, 48, 288, 65) == -1 and rec(-1, 96, 48, 288, 5) == -1
    groups = lambda b: int(_hip.invoke('fgnn_ldpc_nms_backward_workgroups', b))
    assert [groups(b) for b in (0, 1, 67, 512, 513, 10 ** 6)] == [0, 1, 67, 512, 512, 512]
    ws = lambda *a: int(_hip.invoke('fgnn_ldpc_nms_backward_workspace_bytes', *a))
    assert ws(67, 96, 48, 288, 5, 0) == 67 * 2 * 5 * 4 and ws(67, 96, 48, 288, 5, 1) == 67 * 2 * 5 * 48 * 4
    assert ws(4096, 96, 48, 288, 5, 2) == 512 * 2 * 5 * 288 * 4 and ws(1, 96, 48, 288, 5, 3) == -1 and ws(1, 96, 48, 288, 5, -1) == -1

    one = ctypes.c_void_p(16)                      # a non-NULL pointer that is never dereferenced on these paths
    def fwd(llr=one, sb=96, tab=one, w=one, B=4, n=96, m=48, e=288, it=5, share=2, stop=0, x=one, viol=one, iters=one, totals=one,
            record=one, nbytes=4 * 5 * 48 * 12):
        return _hip.invoke('fgnn_ldpc_nms_forward', llr, sb, tab, tab, tab, tab, w, w, B, n, m, e, it, share, stop, x, None, viol, iters,
                           totals, record, nbytes, None)

    def bwd(g=one, llr=one, sb=96, tab=one, w=one, record=one, nbytes=4 * 5 * 48 * 12, B=4, n=96, m=48, e=288, it=5, share=2, ga=one,
            gb=one, gl=one, ws_=one, wbytes=4 * 2 * 5 * 288 * 4):
        return _hip.invoke('fgnn_ldpc_nms_backward', g, llr, sb, tab, tab, tab, tab, w, w, record, nbytes, B, n, m, e, it, share, ga, gb,
                           gl, ws_, wbytes, None)
    for call in (fwd, bwd):
        assert call(n=1025) == _hip.EUNSUPPORTED and call(m=1025) == _hip.EUNSUPPORTED and call(e=16 * 48 + 1) == _hip.EUNSUPPORTED
        assert call(n=0) == _hip.EUNSUPPORTED and call(e=0) == _hip.EUNSUPPORTED
        assert call(it=0) == EINVAL and call(it=65) == EINVAL and b'n_iter' in L.fgnn_last_error()
        assert call(share=3) == EINVAL and call(share=-1) == EINVAL and b'share' in L.fgnn_last_error()
        assert call(sb=-1) == EINVAL and b'stride' in L.fgnn_last_error()
        assert call(B=-1) == EINVAL and call(B=2 ** 31) == EINVAL and b'batch' in L.fgnn_last_error()
        assert call(tab=None) == EINVAL and call(w=None) == EINVAL and b'null' in L.fgnn_last_error()
        assert call(nbytes=4 * 5 * 48 * 12 - 1) == EINVAL and b'record' in L.fgnn_last_error()
        assert call(B=0, n=1025) == _hip.EUNSUPPORTED and call(B=0, it=0) == EINVAL                # sizes are checked even then
    assert fwd(stop=2) == EINVAL and b'stop_early' in L.fgnn_last_error()
    assert fwd(llr=None) == EINVAL and fwd(totals=None) == EINVAL and fwd(record=None) == EINVAL
    assert fwd(stop=1) == EINVAL and b'train mode' in L.fgnn_last_error()                          # totals / record in decode mode
    assert fwd(stop=1, totals=None, record=None, x=None) == EINVAL and fwd(stop=1, totals=None, record=None, viol=None) == EINVAL
    assert fwd(llr=None, tab=None, w=None, x=None, viol=None, iters=None, totals=None, record=None, nbytes=0, B=0) == 0      # empty batch
    assert bwd(g=None) == EINVAL and bwd(record=None) == EINVAL and bwd(ga=None) == EINVAL and bwd(gb=None) == EINVAL and bwd(ws_=None) == EINVAL
    assert bwd(llr=None) == EINVAL and b'clamp' in L.fgnn_last_error()                             # g_llr needs llr
    assert bwd(wbytes=4 * 2 * 5 * 288 * 4 - 1) == EINVAL and b'workspace' in L.fgnn_last_error()
    assert bwd(g=None, llr=None, tab=None, w=None, record=None, ga=None, gb=None, gl=None, ws_=None, nbytes=0, wbytes=0, B=0) == 0


def test_check_nms_args_and_the_module_on_the_host():
    from fgnn_amd.ldpc_code import LdpcCode
    from fgnn_amd.ldpc_nms import LearnedMinSum, check_nms_args, multi_loss
    ok = dict(llr=torch.zeros(5, 96), n_var=96, n_chk=48, n_edges=288, n_iter=5, share='edge', alpha=torch.zeros(5, 288), beta=torch.zeros(5, 288))
    assert check_nms_args(**ok) == (5, 2, 288)
    assert check_nms_args(**dict(ok, share='check', alpha=torch.zeros(5, 48), beta=torch.zeros(5, 48))) == (5, 1, 48)
    assert check_nms_args(**dict(ok, share='iteration', alpha=torch.zeros(5, 1), beta=torch.zeros(5, 1), llr=torch.zeros(0, 96, dtype=torch.float64))) == (0, 0, 1)
    for kw, what in (({'n_iter': 0}, 'n_iter'), ({'n_iter': 65}, 'n_iter'), ({'n_iter': 2.5}, 'n_iter'), ({'n_iter': True}, 'n_iter'),
                     ({'share': 'word'}, 'share'), ({'share': 2}, 'share'), ({'alpha': torch.zeros(5, 48)}, 'alpha'),
                     ({'beta': torch.zeros(4, 288)}, 'beta'), ({'alpha': torch.zeros(5, 288, dtype=torch.float64)}, 'alpha'),
                     ({'beta': np.zeros((5, 288), np.float32)}, 'beta'), ({'llr': torch.zeros(5, 95)}, 'llr'), ({'llr': torch.zeros(96)}, 'llr'),
                     ({'llr': np.zeros((5, 96))}, 'llr'), ({'llr': torch.zeros(5, 96, dtype=torch.int32)}, 'floating')):
        with pytest.raises(ValueError, match=what):
            check_nms_args(**dict(ok, **kw))
    dec = LearnedMinSum(n_iter=4, share='check', alpha=1.0, beta=0.25)          # the built-in code; on the host
    assert list(dec.state_dict()) == ['alpha', 'beta'] and dec.alpha.shape == (4, 48) and dec.alpha.dtype == torch.float32
    assert float(dec.alpha.detach().min()) == 1.0 and float(dec.beta.detach().max()) == 0.25 and dec.alpha.requires_grad and dec.beta.requires_grad
    assert dec.decoder_entry() == {'kind': 'learned-min-sum', 'n_iter': 4, 'share': 'check'}
    assert LearnedMinSum(LdpcCode.gallager(1024, 4, 8, 2), 3).alpha.shape == (3, 4096)       # a code ldpc_train refuses
    with pytest.raises(RuntimeError, match='ROCm'):
        dec(torch.zeros(2, 96))
    with pytest.raises(ValueError, match='llr'):
        dec.decode(torch.zeros(2, 97))
    for kw in ({'n_iter': 0}, {'share': 'all'}, {'alpha': float('nan')}, {'beta': float('inf')}, {'code': LdpcCode.gallager(34, 17, 17, 0)}):
        with pytest.raises(ValueError):
            LearnedMinSum(**kw)
    tables = [getattr(dec, k).numpy() for k in ('col_ptr', 'row_ptr', 'row_edge', 'row_var')]
    assert all(np.array_equal(a, b) and a.dtype == np.int32 for a, b in zip(tables, LO.tables(dec.code.nlist, 48)))
    t, cw = torch.tensor([[[2.0, -1.0]], [[0.5, -3.0]]]), torch.tensor([[0, 1]], dtype=torch.uint8)      # [2, 1, 2]
    want = np.mean([np.log1p(np.exp(-2.0)), np.log1p(np.exp(-1.0)), np.log1p(np.exp(-0.5)), np.log1p(np.exp(-3.0))])
    assert abs(float(multi_loss(t, cw)) - want) < 1e-6


def test_parse_decoder_takes_the_learned_spec_and_the_old_table_holds():
    from fgnn_amd.ldpc_eval import parse_decoder
    for spec, path in (('learned-min-sum:ckpt/a.pt', 'ckpt/a.pt'), ('learned-min-sum:/x/y:z=1:layered.pt', '/x/y:z=1:layered.pt'),
                       ('learned-min-sum:C:\\a.pt', 'C:\\a.pt'), ('learned-min-sum::', ':')):
        assert parse_decoder(spec) == (spec, 'learned', {'path': path})
    for junk in ('learned-min-sum', 'learned-min-sum:', 'learned-min-summer:a', 'learned:a.pt', 'Learned-min-sum:a.pt'):
        with pytest.raises(ValueError):
            parse_decoder(junk)
    # tests/test_ldpc_llr.py::test_parse_decoder_round_trips_and_refuses_junk's table and junk list, as they are there
    for spec, canon, kind, kw in PARSED:
        got = parse_decoder(spec)
        assert got == (canon, kind, kw), spec
        assert parse_decoder(canon) == got
    for junk in JUNK:
        with pytest.raises(ValueError):
            parse_decoder(junk)


def test_learned_checkpoints_are_checked_against_the_code(tmp_path):
    from fgnn_amd.ldpc_code import LdpcCode
    from fgnn_amd.ldpc_nms import LearnedMinSum, load_checkpoint
    from fgnn_amd.ldpc_nms_train import checkpoint_dict, checkpoint_path, lr_sched
    small = LdpcCode.gallager(12, 3, 6, 1)
    dec = LearnedMinSum(small, 3, 'edge', alpha=0.5, beta=0.125)
    opt = torch.optim.Adam(dec.parameters())
    d = checkpoint_dict(dec, opt, torch.optim.lr_scheduler.LambdaLR(opt, lr_sched), 2, 7)
    assert set(d) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt', 'decoder', 'code'}
    assert d['decoder'] == {'kind': 'learned-min-sum', 'n_iter': 3, 'share': 'edge'} and (d['epoch'], d['gcnt']) == (2, 7)
    p = checkpoint_path(str(tmp_path), 'LearnedMinSum', dec, 2, None)
    torch.save(d, p)
    back = load_checkpoint(p, small)
    assert (back.n_iter, back.share) == (3, 'edge') and torch.equal(back.alpha, dec.alpha) and torch.equal(back.beta, dec.beta)
    with pytest.raises(ValueError, match='trained for'):
        load_checkpoint(p, LdpcCode.builtin())
    with pytest.raises(ValueError, match='another incidence'):
        load_checkpoint(p, LdpcCode.gallager(12, 3, 6, 2))
    builtin = checkpoint_dict(LearnedMinSum(), opt, torch.optim.lr_scheduler.LambdaLR(opt, lr_sched), 0, 0)
    assert 'code' not in builtin                                              # the default code's checkpoints carry no entry
    torch.save({'model_state_dict': {}}, p)                                   # an FGNN checkpoint is no learned min-sum decoder
    with pytest.raises(ValueError, match='no learned min-sum'):
        load_checkpoint(p, small)


@pytest.mark.parametrize('name', ('g12', 'builtin', 'g32'))
def test_constant_weights_restate_the_llr_decoders_bit_for_bit(name):
    llr, tb = LG.case(name)[3], tabs(name)
    for algorithm, alpha, beta in (('min-sum', 0.8125, 0.0), ('offset-min-sum', 1.0, 0.5)):
        want = LG.restated(name, algorithm, 'flooding', LG.MS_ITERS)
        for share in SHARES:
            W = NO.weight_count(share, tb)
            got = NO.forward(llr, tb, np.full((LG.MS_ITERS, W), alpha, np.float32), np.full((LG.MS_ITERS, W), beta, np.float32), share, LG.MS_ITERS)
            assert np.array_equal(got['dec_x'], want['x']) and np.array_equal(got['dec_viol'], want['viol'])
            assert np.array_equal(got['dec_iters'], want['iters'])
            assert not np.isnan(want['post']).any() and np.array_equal(LG.bits(got['dec_post']), LG.bits(want['post']))
        assert (want['iters'] < LG.MS_ITERS).any() and (want['viol'] != 0).any()        # early stops and words that never finish


@pytest.mark.parametrize('share', SHARES)
@pytest.mark.parametrize('name', ('g12', 'builtin', 'g32'))
def test_explicit_backward_equals_autograd(name, share):
    alpha, beta = weights(name, share)
    fw = restated(name, share, 'float64')
    rows = np.arange(0, LG.B, 4)                                            # 17 words
    got = NO.backward(fw, g_totals(name), rows)
    want = NO.autograd_backward(words(name), tabs(name), alpha, beta, share, N_ITER[name], g_totals(name), rows)
    err = relative_error(got, want)
    print(name, share, err)
    assert max(err) <= 1e-10
    assert all(np.abs(w).max() > 0 for w in want)
    special = words(name)[:3].copy()                                        # the load rule: no gradient through a clamp or a NaN
    special[0, 1], special[1, 2], special[2, 3] = np.nan, 1e9, -1e9
    fs = NO.forward(special, tabs(name), alpha, beta, share, N_ITER[name], np.float64)
    got = NO.backward(fs, g_totals(name)[:, :3])
    want = NO.autograd_backward(special, tabs(name), alpha, beta, share, N_ITER[name], g_totals(name)[:, :3])
    assert max(relative_error(got, want)) <= 1e-10
    assert got[2][0, 1] == got[2][1, 2] == got[2][2, 3] == 0 and np.count_nonzero(got[2] == 0) == 3


@pytest.mark.parametrize('share', SHARES)
def test_explicit_backward_equals_finite_differences(share):
    """Central differences of sum(g_totals * totals) in float64 on g12, five words; the step 1e-6 is far below the distance to any
    kink on these inputs (asserted: the record does not move under it)."""
    name, rows, h = 'g12', np.arange(5), 1e-6
    alpha, beta = weights(name, share)
    llr, tb, g = words(name)[rows].astype(np.float64), tabs(name), g_totals(name)[:, rows].astype(np.float64)
    fw = restated(name, share, 'float64')
    ga, gb, gl = NO.backward(fw, g_totals(name), rows)

    def value(a, b, x):
        out = NO.torch_forward(torch.from_numpy(x), tb, torch.from_numpy(a), torch.from_numpy(b), share, N_ITER[name]).numpy()
        return float((out * g).sum())
    a64, b64 = alpha.astype(np.float64), beta.astype(np.float64)
    rng = np.random.RandomState(5)
    for arr, grad, pick in ((a64, ga, 0), (b64, gb, 1), (llr, gl, 2)):
        for _ in range(12):
            i = tuple(rng.randint(s) for s in arr.shape)
            up, down = arr.copy(), arr.copy()
            up[i] += h
            down[i] -= h
            args = [a64, b64, llr]
            hi = value(*[up if k == pick else v for k, v in enumerate(args)])
            lo = value(*[down if k == pick else v for k, v in enumerate(args)])
            fd = (hi - lo) / (2 * h)
            assert abs(fd - grad[i]) <= 1e-6 * max(1.0, abs(grad[i])), (share, pick, i, fd, grad[i])


@pytest.mark.parametrize('name', CODES)
def test_gpu_inputs_keep_the_restatement_within_its_cap(name):
    for share in SHARES:
        keep = kept(name, share)
        err = relative_error(restated_backward(name, share, 'float32'), restated_backward(name, share))
        print(name, share, 'left out %d of %d' % ((~keep).sum(), keep.size), 'f32 error', err)
        assert (~keep).mean() <= LEFT_OUT_CAP
        for k, e in zip(D, err):
            assert e <= D[k] * (1 + 1e-3), (k, e)                           # d is what this file says it is
        f32 = restated(name, share)
        assert np.isfinite(f32['totals']).all() and np.abs(f32['totals']).max() < 1e12          # far from the f32 range
        assert (f32['pos'].sum() > 0) and (~f32['pos'] & (np.arange(f32['pos'].shape[2]) >= 0)).any()      # both sides of the relu
    dec = restated(name, 'edge')
    assert (dec['dec_iters'] < N_ITER[name]).any() or name == 'g1024'       # decode mode stops early on some words


if __name__ == '__main__':
    print(restatement_error())
