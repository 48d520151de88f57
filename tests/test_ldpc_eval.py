"""CPU: the LDPC evaluation path's host side (csrc/ldpc_eval.hip, fgnn_ldpc_received_features in csrc/ldpc_datapath.hip,
fgnn_amd/ldpc_eval.py, LdpcDataPath.received_features / make_test_set):

  * both entry points validate their arguments before any launch (no device needed);
  * the Python calls refuse bad shapes and grids with ValueError before anything reaches a device;
  * the numpy restatement the GPU tests hold the kernel to agrees with the reference's own loop body;
  * the new kernels keep everything in registers and LDS (compiler resource report, cross-compiled for gfx950)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ldpc_eval_oracle as EO
import scratch_report as NS

EINVAL = -1                                    # FGNN_EINVAL


def test_received_features_entry_point_validates_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    one = ctypes.c_void_p(16)                  # non-NULL, never dereferenced on these paths
    call = lambda y=one, snr=one, sb=1, sn=0, B=4, nvar=96, nchk=48, dv=3, dc=6, dtype=0, node=one: L.fgnn_ldpc_received_features(
        y, snr, sb, sn, one, one, B, nvar, nchk, dv, dc, dtype, node, one, one, one, None)
    assert call(y=None) == EINVAL and b'null pointer' in L.fgnn_last_error()
    assert call(snr=None) == EINVAL and call(node=None) == EINVAL
    assert call(sb=-1) == EINVAL and call(sn=-1) == EINVAL
    assert call(nvar=1025) == _hip.EUNSUPPORTED and call(dtype=2) == _hip.EUNSUPPORTED and call(dc=0) == _hip.EUNSUPPORTED
    assert call(y=None, snr=None, node=None, B=0) == 0                    # empty batch: nothing to do
    assert call(B=-1) == _hip.EUNSUPPORTED


def test_error_counts_entry_point_validates_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    one = ctypes.c_void_p(16)

    def call(dec=one, dk=0, dsb=48, label=one, lk=0, lsb=96, snr=one, ssb=1, sigma=one, B=4, nbits=48, sg=one, ns=5, bg=one, nb=6,
             counts=one):
        return L.fgnn_ldpc_error_counts(dec, dk, dsb, label, lk, lsb, snr, ssb, sigma, B, nbits, sg, ns, bg, nb, counts, None)

    for kw in ('dec', 'label', 'snr', 'sigma', 'sg', 'bg', 'counts'):
        assert call(**{kw: None}) == EINVAL, kw
    assert b'null pointer' in L.fgnn_last_error()
    assert call(dk=3) == _hip.EUNSUPPORTED and b'decision kind' in L.fgnn_last_error()
    assert call(dk=-1) == _hip.EUNSUPPORTED and call(lk=2) == _hip.EUNSUPPORTED
    assert call(nbits=1025) == _hip.EUNSUPPORTED and call(nbits=0) == _hip.EUNSUPPORTED
    assert call(ns=16, nb=17) == _hip.EUNSUPPORTED and b'classes' in L.fgnn_last_error()
    assert call(ns=0) == _hip.EUNSUPPORTED and call(nb=0) == _hip.EUNSUPPORTED
    assert call(dsb=-1) == EINVAL and call(lsb=-1) == EINVAL and call(ssb=-1) == EINVAL and call(B=-1) == EINVAL
    assert call(dec=None, label=None, snr=None, sigma=None, sg=None, bg=None, counts=None, B=0) == 0
    # the limits themselves are accepted (they only fail at the first null pointer)
    assert call(nbits=1024, ns=16, nb=16, counts=None) == EINVAL and call(dk=2, lk=1, counts=None) == EINVAL


def test_python_calls_refuse_bad_shapes_and_grids_before_any_launch():
    from fgnn_amd.datapath import check_grids, check_received_args
    from fgnn_amd.ldpc_eval import LdpcErrorCounts, check_count_args
    y = torch.zeros(4, 96)
    assert check_received_args(y, torch.zeros(4), torch.float32) == 4
    assert check_received_args(y, torch.zeros(4, 96), torch.bfloat16) == 4
    for yy, snr, dt, what in ((torch.zeros(4, 95), torch.zeros(4), torch.float32, 'received words'),
                              (torch.zeros(96), torch.zeros(1), torch.float32, 'received words'),
                              (y, torch.zeros(5), torch.float32, 'snr_db'), (y, torch.zeros(4, 48), torch.float32, 'snr_db'),
                              (y, torch.zeros(4), torch.float16, 'dtype')):
        with pytest.raises(ValueError, match=what):
            check_received_args(yy, snr, dt)
    assert check_grids((0, 1.5), (0, 2.0)) == ((0.0, 1.5), (0, 2))
    for sg, bg, what in (((), (0,), 'empty'), ((0,), (), 'empty'), (range(16), range(17), 'at most 256'),
                         ((0, float('nan')), (0,), 'finite'), ((0,), (0.5,), 'integers'), ((0,), (2 ** 31,), 'integers'),
                         ((0,), (float('inf'),), 'integers')):
        with pytest.raises(ValueError, match=what):
            check_grids(sg, bg)
    with pytest.raises(ValueError, match='empty'):
        LdpcErrorCounts('cpu', snr_grid=())                   # the grids are checked before the device
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        LdpcErrorCounts('cpu')
    d, lab, s, sb = torch.zeros(4, 48), torch.zeros(4, 96, dtype=torch.int64), torch.zeros(4, 96), torch.zeros(4)
    assert check_count_args(d, lab, s, sb, 48) == 4 and check_count_args(d, lab.byte(), s[:, 0], sb, 48) == 4
    for args, what in (((torch.zeros(4, 47), lab, s, sb, 48), 'decisions'), ((d, torch.zeros(3, 96, dtype=torch.int64), s, sb, 48), 'labels'),
                       ((d, torch.zeros(4, 96), s, sb, 48), 'int64, uint8 or bool'), ((d, lab, torch.zeros(5), sb, 48), 'snr_db'),
                       ((d, lab, s, torch.zeros(4, 1), 48), 'sigma_b'), ((d, lab, s, sb, 0), 'nbits'), ((d, lab, s, sb, 1025), 'nbits')):
        with pytest.raises(ValueError, match=what):
            check_count_args(*args)


def test_restatement_agrees_with_the_reference_loop_body():
    """tests/ldpc_eval_oracle.py against train_ldpc.py:302-323 run literally on torch CPU tensors, over words on and off the grid
    (SNR 2.5, sigma_b 2.7 -> class 2, sigma_b 6 -> no class) and exact +-0 logits."""
    rng = np.random.default_rng(0)
    B = 3000
    pred = rng.standard_normal((B, 48)).astype(np.float32)
    pred[rng.random((B, 48)) < 0.05] = 0.0
    pred[rng.random((B, 48)) < 0.05] = -0.0
    label = rng.integers(0, 2, (B, 96))
    snr = rng.choice(np.array([0, 1, 2, 3, 4, 2.5], np.float32), B)
    sb = rng.choice(np.array([0, 1, 2, 3, 4, 5, 2.7, 6], np.float32), B)
    c = EO.error_counts(pred, 'logits', label, snr, sb)
    acc_cnt, acc_tot, all_correct, tot = EO.reference_loop(torch.from_numpy(pred), torch.from_numpy(label), torch.from_numpy(snr),
                                                           torch.from_numpy(sb).double())
    assert np.array_equal(c[:-1, 0].reshape(5, 6), acc_tot)
    assert np.array_equal((c[:-1, 0] - c[:-1, 1]).reshape(5, 6), acc_cnt)
    assert c[-1, 0] == tot and c[-1, 0] - c[-1, 1] == all_correct
    assert c[:-1, 2].sum() < B and c[-1, 2] == B                          # off-grid words count only overall
    assert np.array_equal(EO.classes([2.0, 2.5, 0.0005, 4.0], [2.7, 2.0, 0.0, 6.0], (0, 1, 2, 3, 4), range(6)), [14, -1, 0, -1])


@pytest.mark.skipif(not os.path.exists(NS.HIPCC), reason='no hipcc')
def test_new_kernels_have_no_scratch():
    bad = []
    for src, subs in (('ldpc_eval.hip', ['ldpc_error_counts_kernel']),
                      ('ldpc_datapath.hip', ['ldpc_received_features_kernel', 'ldpc_features_kernel'])):
        rep = NS.scratch(src)
        assert rep, 'no resource report for %s' % src
        for sub in subs:
            hits = {k: v for k, v in rep.items() if sub in k}
            assert hits, (src, sub)
            bad += ['%s: %s spills %d bytes per lane' % (src, k, v) for k, v in hits.items() if v]
    assert not bad, '\n'.join(bad)
