"""CPU: the max-product baseline's checker and host side (csrc/pgm_bp.hip, fgnn_amd/pgm_datapath.py: solve_bp).

  * the closed-form window message of tests/pgm_bp_oracle.py against the enumeration of all 2^h configurations;
  * without budgets the graph is a chain, a tree: the restated max-product gives the exact MAP after N parallel rounds;
  * the companion header binds beside the main one, whose interface is what it was;
  * argument validation happens before any launch, so it is testable without a device;
  * the kernel keeps everything in registers and LDS (compiler resource report, cross-compiled for gfx950)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pgm_bp_oracle as BO
import pgm_map_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANION = os.path.join(ROOT, 'include', 'fgnn_hip_pgm_bp.h')
NEW = ('fgnn_chain_budget_bp', 'fgnn_chain_budget_bp_lds_bytes')
N, H = 30, 9
EINVAL = -1                                    # FGNN_EINVAL


def test_window_message_closed_form_against_brute_force():
    rng = np.random.default_rng(1)
    for h in range(2, 8):
        for c in range(0, h + 2):
            for _ in range(6):
                delta = rng.uniform(-2, 2, h)
                if rng.random() < 0.3:
                    delta[rng.integers(0, h, 2)] = delta[0]                 # repeated values
                if rng.random() < 0.2:
                    delta = np.round(delta)                                   # zeros and many ties
                got = BO.budget_messages(delta[None], np.array([c]))[0]
                want = BO.budget_messages_brute(delta, c)
                assert np.abs(got - want).max() <= 1e-12, (h, c, delta, got, want)
                if c == 0:
                    assert (got == -BO.FORCE).all() and BO.FORCE == 2.0 ** 20


def test_max_product_is_exact_on_a_chain_without_budgets():
    """Every cap >= h: no window constrains, the graph is a tree, and N undamped parallel rounds carry every message across it."""
    unary, pair, _, _ = PO.sample_draws('pws', 200, N, H, 2, 0)
    caps = np.full((200, N - H + 1), H)
    r = BO.bp(unary, pair, caps, H, max_iter=N, damping=0.0, tol=0.0)
    lab, _ = PO.chain_map(unary, pair, caps, H)
    differ = int((r['labels'] != lab).any(axis=1).sum())
    print('%d of 200 samples differ from the exact MAP' % differ)
    assert differ == 0
    assert (r['iters'] == N).all() and (r['status'] == 3).all()              # tol = 0 never stops early


def test_oracle_statuses_and_start():
    rng = np.random.default_rng(4)
    unary, pair = rng.random((3, 12, 2)).astype(np.float32), rng.random((3, 11, 4)).astype(np.float32)
    caps = np.full((3, 8), 2)
    caps[1, 4] = -1
    r = BO.bp(unary, pair, caps, 5, max_iter=3)
    assert list(r['status']) == [3, 2, 3] and list(r['iters']) == [3, 0, 3]
    assert not r['labels'][1].any() and not r['beliefs'][1].any()
    r0 = BO.bp(unary, pair, caps, 5, max_iter=0)
    u = unary.astype(np.float64)
    assert np.array_equal(r0['beliefs'][[0, 2]], (u[:, :, 1] - u[:, :, 0])[[0, 2]])    # no message yet: the unary log-ratio
    long = BO.bp(unary, pair, caps, 5, max_iter=2000)
    assert (long['status'][[0, 2]] == 0).all() and (long['iters'][[0, 2]] < 2000).all()


def test_companion_header_is_parsed_bound_and_built():
    from fgnn_amd import _hip
    text = open(COMPANION).read()
    assert '#include "fgnn_hip.h"' in text and 'extern "C"' in text
    sig = _hip.signatures(text)
    assert tuple(sig) == NEW == _hip.PGM_BP
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
    assert [n for n, _ in sig[NEW[0]][1]] == ['unary', 'unary_sb', 'pair', 'pair_sb', 'caps', 'caps_sb', 'B', 'N', 'h', 'max_iter',
                                              'tol', 'damping', 'labels', 'beliefs', 'status', 'iters', 'stream']
    args = dict(sig[NEW[0]][1])
    assert args['tol'] is ctypes.c_double and args['damping'] is ctypes.c_double and args['B'] is ctypes.c_int64
    assert args['unary'] is _hip.DevicePointer and args['stream'] is _hip.DevicePointer
    assert text.count('No counterpart in the reference') == 2        # each prototype says why it exists


def test_library_bp_footprint_and_validation_without_a_device():
    from fgnn_amd import _hip
    L = _hip.lib()
    q = lambda n, h: int(_hip.invoke('fgnn_chain_budget_bp_lds_bytes', n, h))
    W = N - H + 1
    assert q(N, H) == (8 * (2 * N + 2 * (N - 1) + 2 * W * H) + 16 * (N - 1) + 4 * W + 15) // 16 * 16
    for h in range(2, 14):
        for n in range(h, 129):
            assert 0 < q(n, h) <= 64 * 1024, (n, h)
    for n, h in ((30, 14), (30, 1), (8, 9)):
        assert q(n, h) == -1
    assert b'outside 2..13' in (q(30, 14), L.fgnn_last_error())[1]
    assert q(20000, 13) == -1 and b'LDS' in L.fgnn_last_error()
    one = ctypes.c_void_p(16)                      # a non-NULL pointer that is never dereferenced on these paths
    bp = lambda u=one, B=4, n=N, h=H, it=200, tol=1e-6, damping=0.5, lab=one: _hip.invoke(
        'fgnn_chain_budget_bp', u, 2 * n, one, 0, one, 0, B, n, h, it, tol, damping, lab, None, None, None, None)
    assert bp(h=14) == _hip.EUNSUPPORTED and bp(n=8) == _hip.EUNSUPPORTED
    assert bp(u=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert bp(lab=None) == EINVAL
    assert bp(it=-1) == EINVAL and b'max_iter' in L.fgnn_last_error()
    assert bp(tol=float('nan')) == EINVAL and bp(tol=-1.0) == EINVAL and b'tol' in L.fgnn_last_error()
    for d in (1.0, -0.1, float('nan'), float('inf')):
        assert bp(damping=d) == EINVAL and b'damping' in L.fgnn_last_error()
    assert bp(B=-1) == EINVAL
    assert bp(u=None, lab=None, B=0) == 0                               # empty batch: nothing to do


def _host_path(device='cuda:0'):
    import torch
    from fgnn_amd import PgmDataPath
    path = PgmDataPath.__new__(PgmDataPath)                                   # host side only: no device is touched
    path.N, path.h, path.device = N, H, torch.device(device)
    return path


def test_solve_bp_validates_on_the_host():
    import torch
    path = _host_path()
    u, p, c = torch.zeros(2, N, 2), torch.zeros(N - 1, 4), 3
    for kw, what in (({'damping': 1.0}, 'damping'), ({'damping': -0.25}, 'damping'), ({'damping': float('nan')}, 'damping'),
                     ({'max_iter': -1}, 'max_iter'), ({'tol': float('nan')}, 'tol'), ({'tol': float('inf')}, 'tol'),
                     ({'tol': -1e-6}, 'tol')):
        with pytest.raises(ValueError, match=what):
            path.solve_bp(u, p, c, **kw)
    with pytest.raises(ValueError, match='unary'):
        path.solve_bp(torch.zeros(2, N, 3), p, c)
    with pytest.raises(ValueError, match='pair'):
        path.solve_bp(u, torch.zeros(N, 4), c)
    with pytest.raises(ValueError, match='caps'):
        path.solve_bp(u, p, torch.zeros(N - H, dtype=torch.int32))
    with pytest.raises(ValueError, match='caps'):
        path.solve_bp(u, p, torch.zeros(N - H + 1))
    for kw, what in (({'family': 'chains'}, 'family'), ({'B': -1}, 'batch'), ({'transition': (0, 1, 2)}, 'transition')):
        a = dict(B=4, family='hops')
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            path.sample(bp_label=True, **a)


def test_solve_bp_needs_a_device():
    import torch
    from fgnn_amd import PgmDataPath
    with pytest.raises(RuntimeError):
        PgmDataPath('cpu', N, H)
    with pytest.raises(RuntimeError):                                          # host tensors never reach the library
        _host_path('cpu').solve_bp(torch.zeros(2, N, 2), torch.zeros(N - 1, 4), 3)
    from fgnn_amd.pgm_eval import evaluate
    with pytest.raises(ValueError, match='bp_args'):
        evaluate(None, (), (torch.zeros(2, 2, N, 1), torch.zeros(2, N, dtype=torch.int64), None), 'raw', bp=True,
                 bp_args={'eta': 0.1})


@pytest.mark.skipif(not os.path.exists(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')), reason='no hipcc')
def test_bp_kernel_has_no_scratch():
    from scratch_report import scratch
    rep = scratch('pgm_bp.hip')
    hits = {k: v for k, v in rep.items() if 'chain_budget_bp_kernel' in k}
    assert len(hits) == 1, rep
    assert not any(hits.values()), hits
