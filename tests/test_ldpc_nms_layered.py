"""CPU: the layered learned min-sum LDPC decoder's checker and host side (csrc/ldpc_nms_layered.hip,
include/fgnn_hip_ldpc_nms_layered.h, fgnn_amd/ldpc_nms.py's ``schedule='layered'``, ldpc_nms_train's ``schedule``), and the inputs
tests/test_ldpc_nms_layered_gpu.py shares with this file.

  * the companion header binds beside the others, whose interfaces are what they were;
  * argument validation and the LDS query happen before any launch, so they are testable without a device;
  * the f32 restatement tests/ldpc_nms_layered_oracle.py with constant weights is tests/ldpc_llr_oracle.py's layered min-sum / offset
    min-sum bit for bit;
  * its explicit backward recursion equals torch autograd's over a float64 layered forward, a degree-1 check included;
  * the inputs of the GPU comparison: at most 5 % of the words have a record that differs between the restatement's two precisions,
    and the restatement's own f32 error is what ``D`` says.

Cases (``code``, ``words``, ``weights``, ``g_totals``): tests/test_ldpc_nms.py's for g12, builtin, g32 and g1024; 'g64' =
gallager(64, 3, 16, 1), the degree-16 case of the backward comparison (67 words at 3 dB, 5 iterations; g32's layered records differ
between f32 and f64 on up to 37 of 67 words, far over the cap: a dense 32 x 32 code's ties break differently in the two precisions);
'w1024' = gallager(1024, 2, 2, 3), whose two layers hold 512 checks each, more than the 256 threads; 'irregular', a hand-made matrix
with a degree-1 check, which ``LdpcCode`` refuses, so its tables are built here."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import ldpc_llr_oracle as LO
import ldpc_nms_layered_oracle as YO
import test_ldpc_llr_gpu as LG
import test_ldpc_nms as NC
from ldpc_decoder_cases import received

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANION = os.path.join(ROOT, 'include', 'fgnn_hip_ldpc_nms_layered.h')
NEW = ('fgnn_ldpc_nms_layered_forward', 'fgnn_ldpc_nms_layered_backward', 'fgnn_ldpc_nms_layered_lds_bytes')
EINVAL = -1                                    # FGNN_EINVAL

SHARES = YO.SHARES
FORWARD_CODES = ('g12', 'builtin', 'g32', 'g1024', 'w1024')
BACKWARD_CODES = ('g12', 'builtin', 'g1024', 'g64')
N_ITER = dict(NC.N_ITER, g64=5, w1024=3, irregular=4)
# d per output tensor: the largest |g_f32 - g_f64| / max |g_f64| between the restatement's own two precisions (``YO.backward`` on
# ``YO.forward`` in float32 and in float64) over every (code, share) of BACKWARD_CODES (the irregular case stays below it, asserted
# with the others), on the words whose two records agree;
# measured on the CPU by ``restatement_error`` (python tests/test_ldpc_nms_layered.py prints it).  The GPU bound is 4 d.
D = {'g_alpha': 6.890e-07, 'g_beta': 3.033e-07, 'g_llr': 2.656e-07}      # measured; no word is left out in any case
LEFT_OUT_CAP = 0.05

# H rows over 6 variables: {0,1,3}, {1,2,4}, {0,4,5}, {2,3,5}, {5}; the layers are not in index order
IRREGULAR_NLIST = np.array([[0, 2, -1], [0, 1, -1], [1, 3, -1], [0, 3, -1], [1, 2, -1], [2, 3, 4]])
IRREGULAR_LAYERS = (np.array([0, 2, 3, 4, 5], np.int32), np.array([0, 4, 1, 2, 3], np.int32))


@functools.lru_cache(maxsize=None)
def code(name):
    from fgnn_amd.ldpc_code import LdpcCode
    if name in NC.CODES:
        return LG.case(name)[0]
    return {'g64': lambda: LdpcCode.gallager(64, 3, 16, 1), 'w1024': lambda: LdpcCode.gallager(1024, 2, 2, 3)}[name]()


@functools.lru_cache(maxsize=None)
def tabs(name):
    if name == 'irregular':
        return LO.tables(IRREGULAR_NLIST, 5)
    return LO.tables(code(name).nlist, code(name).n_chk)


def layers(name):
    return IRREGULAR_LAYERS if name == 'irregular' else code(name).layers()


@functools.lru_cache(maxsize=None)
def words(name):
    if name in NC.CODES:
        return NC.words(name)
    if name == 'g64':
        return received(code(name), 1234, (3.0, 3.0), 67)
    if name == 'w1024':
        return received(code(name), 1235, (3.0, 3.0), 5)
    llr = (np.random.RandomState(1236).standard_normal((9, 6)) * 2.0 + 1.0).astype(np.float32)      # irregular
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def weights(name, share):
    """(alpha, beta) [n_iter, W] f32: alpha in [0.3, 1.2], beta in [0, 0.4], one draw per weight."""
    if name in NC.CODES:
        return NC.weights(name, share)
    seed = {'g64': 7, 'w1024': 3100, 'irregular': 3200}[name] + SHARES.index(share)
    rng = np.random.RandomState(seed)
    W = YO.weight_count(share, tabs(name))
    alpha = rng.uniform(0.3, 1.2, (N_ITER[name], W)).astype(np.float32)
    beta = rng.uniform(0.0, 0.4, (N_ITER[name], W)).astype(np.float32)
    alpha.setflags(write=False)
    beta.setflags(write=False)
    return alpha, beta


@functools.lru_cache(maxsize=None)
def g_totals(name):
    if name in NC.CODES:
        return NC.g_totals(name)
    seed = 4200 + ('g64', 'w1024', 'irregular').index(name)
    g = np.random.RandomState(seed).standard_normal((N_ITER[name],) + words(name).shape).astype(np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def restated(name, share, dtype='float32'):
    """The restatement's train-mode forward on ``words(name)`` with ``weights(name, share)``: computed once, shared, never written."""
    alpha, beta = weights(name, share)
    return YO.forward(words(name), tabs(name), layers(name), alpha, beta, share, N_ITER[name], np.dtype(dtype))


@functools.lru_cache(maxsize=None)
def kept(name, share):
    """[B] bool: the words whose f32 and f64 records agree in every field (a flipped minimum is another function, not an error)."""
    return YO.same_record(restated(name, share), restated(name, share, 'float64'))


@functools.lru_cache(maxsize=None)
def restated_backward(name, share, dtype='float64'):
    """(g_alpha, g_beta, g_llr) of the explicit recursion on the kept words."""
    return YO.backward(restated(name, share, dtype), g_totals(name), kept(name, share))


relative_error = NC.relative_error


def restatement_error():
    """({tensor: d}, the largest fraction of words left out in any case)."""
    d, out = dict.fromkeys(D, 0.0), 0.0
    for name in BACKWARD_CODES:
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
    assert tuple(sig) == NEW == _hip.LDPC_NMS_LAYERED
    assert not set(NEW) & set(_hip.EXPORTS) and not set(NEW) & set(_hip.SIGNATURES) and _hip.ABI_VERSION == 15
    for other in ('LDPC_TRAIN', 'PGM_BP', 'LDPC_CODE', 'LDPC_LLR', 'LDPC_NMS', 'LDPC_OSD', 'WGRAD'):       # in no other table
        assert not set(NEW) & set(getattr(_hip, other))
        assert all(_hip.COMPANIONS[n][2] != 'fgnn_hip_ldpc_nms_layered.h' for n in getattr(_hip, other))
    assert _hip.LDPC_NMS == NC.NEW and tuple(_hip.signatures(open(NC.COMPANION).read())) == NC.NEW       # what they were
    for path in (_hip.HEADER_PATH, NC.COMPANION):
        assert not any(re.search(r'\b%s\b' % name, open(path).read()) for name in NEW)
    L = _hip.lib()
    for name in NEW:
        fn = getattr(L, name)                                        # exported by the built library ...
        restype, params = sig[name]
        assert fn.restype is restype                                 # ... and bound with the parsed types
        assert list(fn.argtypes) == [t for _, t in params] and _hip.COMPANIONS[name][:2] == sig[name]
    assert [sig[n][0] for n in NEW] == [ctypes.c_int32] * 2 + [ctypes.c_int64]
    flooding = _hip.signatures(open(NC.COMPANION).read())
    for new, old in zip(NEW[:2], NC.NEW[:2]):                        # the flooding call's parameters with the layer tables behind row_var
        want = [n for n, _ in flooding[old][1]]
        at = want.index('row_var') + 1
        assert [n for n, _ in sig[new][1]] == want[:at] + ['layer_ptr', 'layer_chk', 'n_layers'] + want[at:]
        args, ref = dict(sig[new][1]), dict(flooding[old][1])
        assert all(args[k] is ref[k] for k in ref)
        assert args['layer_ptr'] is _hip.DevicePointer and args['layer_chk'] is _hip.DevicePointer and args['n_layers'] is ctypes.c_int32
    assert [n for n, _ in sig[NEW[2]][1]] == ['N', 'M', 'E', 'backward']
    assert text.count('No counterpart in the reference') >= len(NEW)  # each prototype says why it exists


def test_lds_query_and_validation_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    lds = lambda n, m, e, bwd: int(_hip.invoke('fgnn_ldpc_nms_layered_lds_bytes', n, m, e, bwd))
    r16 = lambda v: (v + 15) // 16 * 16
    # forward: f32 R [E], T [N], prior [N], the packed row table [E], 4 wave counts; 16-bit row_ptr, col_ptr, layer_chk, layer_ptr.
    # backward: f32 gR [E], gT [N], the row table, 8 wave sums; 16-bit row_ptr, layer_chk, layer_ptr.
    fwd_bytes = lambda n, m, e: r16(4 * (2 * e + 2 * n) + 16) + r16(2 * ((m + 1) + (n + 1) + m + (m + 1)))
    bwd_bytes = lambda n, m, e: r16(4 * (2 * e + n) + 32) + r16(2 * ((m + 1) + m + (m + 1)))
    for n, m, e in ((96, 48, 288), (12, 6, 36), (1024, 512, 4096), (1024, 1024, 16384), (1024, 1024, 2048), (1, 1, 1), (6, 5, 13)):
        assert lds(n, m, e, 0) == fwd_bytes(n, m, e) and lds(n, m, e, 1) == bwd_bytes(n, m, e), (n, m, e)
        # what the kernels carve, placed one behind the other, fits
        assert 4 * (2 * e + 2 * n) + 16 + 2 * ((m + 1) + (n + 1) + m + (m + 1)) <= lds(n, m, e, 0)
        assert 4 * (2 * e + n) + 32 + 2 * ((m + 1) + m + (m + 1)) <= lds(n, m, e, 1)
        assert lds(n, m, e, 1) % 16 == 0                                           # the partial behind it is f32
    assert lds(96, 48, 288, 0) < 4096 and lds(1024, 1024, 16384, 0) <= 160 * 1024         # sized by the code; within a CU's LDS
    assert lds(1024, 512, 4096, 1) < int(_hip.invoke('fgnn_ldpc_nms_lds_bytes', 1024, 512, 4096, 1))      # no prior, no col_ptr
    for n, m, e in ((1025, 48, 288), (0, 48, 288), (96, 1025, 288), (96, 0, 288), (96, 48, 0), (96, 48, -1), (1024, 1024, 16385),
                    (96, 48, 16 * 48 + 1), (8, 48, 16 * 8 + 1)):
        assert lds(n, m, e, 0) == -1 and lds(n, m, e, 1) == -1, (n, m, e)
    assert b'variables' in (lds(1025, 48, 288, 0), L.fgnn_last_error())[1]

    one = ctypes.c_void_p(16)                      # a non-NULL pointer that is never dereferenced on these paths
    def fwd(llr=one, sb=96, tab=one, lay=one, nl=3, w=one, B=4, n=96, m=48, e=288, it=5, share=2, stop=0, x=one, viol=one, iters=one,
            totals=one, record=one, nbytes=4 * 5 * 48 * 12):
        return _hip.invoke('fgnn_ldpc_nms_layered_forward', llr, sb, tab, tab, tab, tab, lay, lay, nl, w, w, B, n, m, e, it, share, stop,
                           x, None, viol, iters, totals, record, nbytes, None)

    def bwd(g=one, llr=one, sb=96, tab=one, lay=one, nl=3, w=one, record=one, nbytes=4 * 5 * 48 * 12, B=4, n=96, m=48, e=288, it=5,
            share=2, ga=one, gb=one, gl=one, ws_=one, wbytes=4 * 2 * 5 * 288 * 4):
        return _hip.invoke('fgnn_ldpc_nms_layered_backward', g, llr, sb, tab, tab, tab, tab, lay, lay, nl, w, w, record, nbytes, B, n, m,
                           e, it, share, ga, gb, gl, ws_, wbytes, None)
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
        assert call(nl=0) == EINVAL and call(nl=49) == EINVAL and call(nl=-1) == EINVAL and b'n_layers' in L.fgnn_last_error()      # 0 and M + 1
        assert call(B=0, nl=0) == EINVAL and call(B=0, nl=49) == EINVAL
        assert call(lay=None) == EINVAL and b'layer table' in L.fgnn_last_error()
        assert call(m=1, n=1, e=1, nl=2, sb=1) == EINVAL and b'n_layers' in L.fgnn_last_error()   # M = 1: one layer at most
    assert fwd(stop=2) == EINVAL and b'stop_early' in L.fgnn_last_error()
    assert fwd(llr=None) == EINVAL and fwd(totals=None) == EINVAL and fwd(record=None) == EINVAL
    assert fwd(stop=1) == EINVAL and b'train mode' in L.fgnn_last_error()                          # totals / record in decode mode
    assert fwd(stop=1, totals=None, record=None, x=None) == EINVAL and fwd(stop=1, totals=None, record=None, viol=None) == EINVAL
    assert fwd(llr=None, tab=None, lay=None, w=None, x=None, viol=None, iters=None, totals=None, record=None, nbytes=0, B=0) == 0      # empty batch
    assert fwd(llr=None, tab=None, lay=None, w=None, x=None, viol=None, iters=None, totals=None, record=None, nbytes=0, B=0, nl=48) == 0
    assert bwd(g=None) == EINVAL and bwd(record=None) == EINVAL and bwd(ga=None) == EINVAL and bwd(gb=None) == EINVAL and bwd(ws_=None) == EINVAL
    assert bwd(llr=None) == EINVAL and b'clamp' in L.fgnn_last_error()                             # g_llr needs llr
    assert bwd(wbytes=4 * 2 * 5 * 288 * 4 - 1) == EINVAL and b'workspace' in L.fgnn_last_error()
    assert bwd(g=None, llr=None, tab=None, lay=None, w=None, record=None, ga=None, gb=None, gl=None, ws_=None, nbytes=0, wbytes=0, B=0) == 0


def test_the_wide_code_is_what_the_gpu_file_needs_it_to_be():
    c = code('w1024')
    lp, lc = c.layers()
    assert (c.n_var, c.n_chk) == (1024, 1024) and list(np.diff(lp)) == [512, 512] and c.require_llr_decoder() is c
    assert sorted(lc) == list(range(1024))
    c = code('g64')
    assert (c.n_var, c.n_chk, c.dc) == (64, 12, 16) and c.require_llr_decoder() is c
    col_ptr, row_ptr, row_edge, row_var = tabs('irregular')
    assert [list(row_var[row_ptr[m]:row_ptr[m + 1]]) for m in range(5)] == [[0, 1, 3], [1, 2, 4], [0, 4, 5], [2, 3, 5], [5]]
    lp, lc = IRREGULAR_LAYERS
    for k in range(4):                                                          # no two checks of a layer share a variable
        vs = np.concatenate([row_var[row_ptr[m]:row_ptr[m + 1]] for m in lc[lp[k]:lp[k + 1]]])
        assert len(set(vs)) == len(vs)


@pytest.mark.parametrize('name', ('g12', 'builtin', 'g32', 'g1024'))
def test_constant_weights_restate_the_layered_llr_decoders_bit_for_bit(name):
    llr, tb = LG.case(name)[3], tabs(name)
    for algorithm, alpha, beta in (('min-sum', 0.8125, 0.0), ('offset-min-sum', 1.0, 0.5)):
        want = LG.restated(name, algorithm, 'layered', LG.MS_ITERS)
        for share in SHARES if name != 'g1024' else ('check',):
            W = YO.weight_count(share, tb)
            got = YO.forward(llr, tb, layers(name), np.full((LG.MS_ITERS, W), alpha, np.float32), np.full((LG.MS_ITERS, W), beta, np.float32),
                             share, LG.MS_ITERS)
            assert np.array_equal(got['dec_x'], want['x']) and np.array_equal(got['dec_viol'], want['viol'])
            assert np.array_equal(got['dec_iters'], want['iters'])                # every word, whichever iteration it stops at
            nan = np.isnan(want['post'])                                            # (g32 overflows: NaN places are compared as places)
            assert np.array_equal(np.isnan(got['dec_post']), nan)
            assert np.array_equal(LG.bits(got['dec_post'])[~nan], LG.bits(want['post'])[~nan])
        assert (want['iters'] < LG.MS_ITERS).any() and len(set(want['iters'])) > 1      # early stops, at more than one iteration count


@pytest.mark.parametrize('share', SHARES)
@pytest.mark.parametrize('name', ('g12', 'builtin', 'irregular'))
def test_explicit_backward_equals_autograd(name, share):
    alpha, beta = weights(name, share)
    fw = restated(name, share, 'float64')
    rows = np.arange(0, len(words(name)), 4)
    got = YO.backward(fw, g_totals(name), rows)
    want = YO.autograd_backward(words(name), tabs(name), layers(name), alpha, beta, share, N_ITER[name], g_totals(name), rows)
    err = relative_error(got, want)
    print(name, share, err)
    assert max(err) <= 1e-12
    assert all(np.abs(w).max() > 0 for w in want)
    special = words(name)[:3].copy()                                        # the load rule: no gradient through a clamp or a NaN
    special[0, 1], special[1, 2], special[2, 3] = np.nan, 1e9, -1e9
    fs = YO.forward(special, tabs(name), layers(name), alpha, beta, share, N_ITER[name], np.float64)
    got = YO.backward(fs, g_totals(name)[:, :3])
    want = YO.autograd_backward(special, tabs(name), layers(name), alpha, beta, share, N_ITER[name], g_totals(name)[:, :3])
    assert max(relative_error(got, want)) <= 1e-12
    assert got[2][0, 1] == got[2][1, 2] == got[2][2, 3] == 0 and np.count_nonzero(got[2] == 0) == 3


def test_the_layered_forward_is_not_the_flooding_one():
    import ldpc_nms_oracle as NO
    alpha, beta = weights('builtin', 'edge')
    flooding = NO.forward(words('builtin'), tabs('builtin'), alpha, beta, 'edge', N_ITER['builtin'])
    assert not np.array_equal(flooding['totals'][0], restated('builtin', 'edge')['totals'][0])


@pytest.mark.parametrize('name', BACKWARD_CODES + ('irregular',))
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
        assert f32['pos'].any() and (~f32['pos']).any()                     # both sides of the relu


def test_the_module_and_the_trainer_on_the_host(tmp_path):
    from fgnn_amd.ldpc_code import LdpcCode
    from fgnn_amd.ldpc_nms import LearnedMinSum, load_checkpoint
    from fgnn_amd.ldpc_nms_train import checkpoint_dict, checkpoint_path, lr_sched, train
    for bad in ('Layered', 'serial', None, 1, ''):
        with pytest.raises(ValueError, match='schedule'):
            LearnedMinSum(n_iter=3, schedule=bad)
    small = LdpcCode.gallager(12, 3, 6, 1)
    flood, lay = LearnedMinSum(small, 3, 'edge', alpha=0.5, beta=0.125), LearnedMinSum(small, 3, 'edge', alpha=0.5, beta=0.125, schedule='layered')
    assert LearnedMinSum(small, 3).schedule == 'flooding' and lay.schedule == 'layered'
    assert list(lay.state_dict()) == ['alpha', 'beta'] == list(flood.state_dict())
    assert flood.decoder_entry() == {'kind': 'learned-min-sum', 'n_iter': 3, 'share': 'edge'}                       # as it was
    assert lay.decoder_entry() == {'kind': 'learned-min-sum', 'n_iter': 3, 'share': 'edge', 'schedule': 'layered'}
    assert not hasattr(flood, 'layer_ptr')
    for got, want in zip((lay.layer_ptr, lay.layer_chk), small.layers()):
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert 'layered' in repr(lay) and 'schedule' not in repr(flood)
    with pytest.raises(RuntimeError, match='ROCm'):
        lay(torch.zeros(2, 12))
    assert checkpoint_path('out', 'LearnedMinSum', flood, 5, None) == os.path.join('out', 'LearnedMinSum_edge_3_epoches_5_snr_None.pt')
    assert checkpoint_path('out', 'LearnedMinSum', lay, 5, 2) == os.path.join('out', 'LearnedMinSum_edge_layered_3_epoches_5_snr_2.pt')

    opt = torch.optim.Adam(lay.parameters())
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_sched)
    with torch.no_grad():
        lay.alpha.mul_(torch.linspace(0.5, 1.5, lay.alpha.numel()).reshape(lay.alpha.shape))
    d = checkpoint_dict(lay, opt, sched, 2, 7)
    assert d['decoder'] == lay.decoder_entry() and set(d) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt', 'decoder', 'code'}
    p = checkpoint_path(str(tmp_path), 'LearnedMinSum', lay, 2, None)
    torch.save(d, p)
    back = load_checkpoint(p, small)
    assert (back.n_iter, back.share, back.schedule) == (3, 'edge', 'layered') and torch.equal(back.alpha, lay.alpha) and torch.equal(back.beta, lay.beta)
    assert torch.equal(back.layer_chk, lay.layer_chk)
    q = checkpoint_path(str(tmp_path), 'LearnedMinSum', flood, 2, None)
    torch.save(checkpoint_dict(flood, opt, sched, 2, 7), q)
    assert p != q and load_checkpoint(q, small).schedule == 'flooding'          # no 'schedule' entry: flooding
    # resume: the checkpoint's decoder entry must be the arguments', the schedule included (refused before anything reaches the device)
    for path, schedule in ((p, 'flooding'), (q, 'layered')):
        with pytest.raises(ValueError, match='holds'):
            train(n_epochs=3, n_iter=3, share='edge', model_path=path, code=small, schedule=schedule, device='cuda:0', out_dir=str(tmp_path))
    with pytest.raises(ValueError, match='schedule'):
        train(n_epochs=1, schedule='both', device='cuda:0', out_dir=str(tmp_path))


if __name__ == '__main__':
    print(restatement_error())
