"""CPU: the synthetic-PGM data path's checker and host side (csrc/pgm_datapath.hip, fgnn_amd/pgm_datapath.py).

  * the numpy DP (tests/pgm_map_oracle.py), which the GPU tests hold the kernel to bit for bit, equals brute-force enumeration;
  * argument validation happens before any launch, so it is testable without a device;
  * the new kernels keep everything in registers and LDS (compiler resource report, cross-compiled for gfx950)."""
import os

import numpy as np
import pytest
import torch

import pgm_map_oracle as PO
from scratch_report import HIPCC, scratch


def _dyadic(rng, shape, lo, hi):
    """Multiples of 2^-24 in [lo, hi): every f64 sum of a few dozen of them is exact, whatever the order."""
    return (lo + (hi - lo) * rng.integers(0, 1 << 24, shape) / float(1 << 24)).astype(np.float32)


@pytest.mark.parametrize('h', [2, 3, 5, 9])
@pytest.mark.parametrize('shared_pair', [True, False], ids=['shared_pair', 'per_sample_pair'])
def test_oracle_dp_equals_brute_force(h, shared_pair):
    rng = np.random.default_rng(100 * h + shared_pair)
    for N in sorted({h, h + 1, 11, 14} - {n for n in (11, 14) if n < h}):
        B = 24
        unary = _dyadic(rng, (B, N, 2), 0, 1)
        pair = _dyadic(rng, (1 if shared_pair else B, N - 1, 4), -1, 1)
        pair = np.broadcast_to(pair, (B, N - 1, 4))
        caps = rng.integers(0, h + 1, (B, N - h + 1))               # 0 (all zeros forced) .. h (no constraint)
        lab, obj = PO.chain_map(unary, pair, caps, h)
        assert PO.feasible(lab, caps, h).all()
        for b in range(B):
            best, argmaxes, _, score = PO.brute_force(unary[b], pair[b], caps[b], h)
            assert obj[b] == best, (N, h, b)
            i = int((lab[b] << np.arange(N)).sum())
            assert score[i] == best                                   # the DP's labels reach the optimum ...
            if len(argmaxes) == 1:
                assert np.array_equal(lab[b], argmaxes[0])            # ... and are the optimum where it is unique


def test_oracle_dp_without_budgets_is_plain_viterbi():
    """cap >= h removes the budgets: the DP over 2^(h-1) states equals a two-state Viterbi with the same tie rule."""
    rng = np.random.default_rng(7)
    B, N, h = 64, 20, 5
    unary, pair = _dyadic(rng, (B, N, 2), 0, 1), _dyadic(rng, (B, N - 1, 4), -1, 1)
    lab, obj = PO.chain_map(unary, pair, np.full((B, N - h + 1), h), h)
    lab2, obj2 = PO.chain_map(unary, pair, np.full((B, N - 1), 2), 2)
    assert np.array_equal(obj, obj2) and np.array_equal(lab, lab2)


def test_oracle_ties_go_to_zeros():
    """All potentials zero: every feasible assignment ties; the rule (d = 0, lowest final state) gives all zeros."""
    lab, obj = PO.chain_map(np.zeros((1, 12, 2)), np.zeros((1, 11, 4)), np.full((1, 8), 2), 5)
    assert not lab.any() and obj[0] == 0.0


def test_library_footprint_query():
    from fgnn_amd import _hip
    L = _hip.lib()
    q = lambda N, h: int(L.fgnn_chain_budget_map_lds_bytes(N, h))
    # 2 S doubles of scores, N S / 8 bytes of backpointers (a 64-bit word per row at least), unary 2N, pair 4(N-1), caps N
    assert q(30, 9) == 16 * 256 + 30 * 4 * 8 + 4 * (60 + 116 + 30) + 8
    assert q(40, 13) == 16 * 4096 + 40 * 64 * 8 + 4 * (80 + 156 + 40) + 0
    assert q(16, 3) == 16 * 4 + 16 * 8 + 4 * (32 + 60 + 16)
    for N, h in ((30, 14), (30, 1), (8, 9), (200, 13)):
        assert q(N, h) == -1
    assert q(182, 13) > 0 and q(183, 13) == -1                         # 160 KiB per workgroup


def test_host_validation_without_a_device():
    from fgnn_amd import PgmDataPath
    from fgnn_amd import pgm_datapath as pd
    with pytest.raises(ValueError, match='outside 2..13'):
        PgmDataPath('cpu', 30, 14)
    with pytest.raises(ValueError, match='shorter than the window'):
        PgmDataPath('cpu', 8, 9)
    with pytest.raises(ValueError, match='LDS'):
        PgmDataPath('cpu', 200, 13)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        PgmDataPath('cpu', 30, 9)
    N, h = 30, 9
    u, p, c = torch.zeros(4, N, 2), torch.zeros(N - 1, 4), torch.zeros(N - h + 1, dtype=torch.int32)
    B, uu, pp, cc = pd.check_solve_args(u, p, c, N, h)
    assert B == 4 and tuple(pp.shape) == (1, N - 1, 4) and tuple(cc.shape) == (1, N - h + 1)
    B, _, pp, cc = pd.check_solve_args(u, torch.zeros(4, N - 1, 2, 2), 5, N, h)
    assert tuple(pp.shape) == (4, N - 1, 4) and tuple(cc.shape) == (1, N - h + 1) and int(cc[0, 0]) == 5
    bad = [(torch.zeros(4, N, 3), p, c, 'unary'), (torch.zeros(N, 2), p, c, 'unary'), (u, torch.zeros(N, 4), c, 'pair'),
           (u, torch.zeros(3, N - 1, 4), c, 'pair'), (u, p, torch.zeros(N - h, dtype=torch.int32), 'caps'),
           (u, p, torch.zeros(5, N - h + 1, dtype=torch.int32), 'caps'), (u, p, torch.zeros(N - h + 1), 'caps must be integers')]
    for uu, pp, cc, what in bad:
        with pytest.raises(ValueError, match=what):
            pd.check_solve_args(uu, pp, cc, N, h)
    with pytest.raises(ValueError, match='outside 2..13'):
        pd.check_solve_args(torch.zeros(4, N, 2), torch.zeros(N - 1, 4), torch.zeros(N - 13, dtype=torch.int32), N, 14)


def test_philox_word_packing():
    """Word w of sample b is word w & 3 of the block with counter (b, w >> 2, offset): blocks of distinct samples, positions and
    offsets differ; the same (seed, offset) gives the same words whatever the batch size."""
    a = PO.philox_words(8, 119, seed=3, offset=5)
    assert a.dtype == np.uint32 and a.shape == (8, 119)
    assert np.array_equal(PO.philox_words(3, 119, 3, 5), a[:3])
    assert not np.array_equal(PO.philox_words(8, 119, 3, 6), a)
    assert len(np.unique(a)) > 0.99 * a.size


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_pgm_kernels_have_no_scratch():
    rep = scratch('pgm_datapath.hip')
    hits = {k: v for k, v in rep.items() if 'chain_budget_map_kernel' in k}
    assert len(hits) == 2, rep                                          # the solver and the sampler instance
    assert not any(hits.values()), hits
