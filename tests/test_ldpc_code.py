"""CPU: ``LdpcCode`` (fgnn_amd/ldpc_code.py), the host side of the layers that take one, and the companion header of the two W-word
entry points (include/fgnn_hip_ldpc_code.h; csrc/ldpc_code.hip).

  * the Gallager test codes are regular, K + P = N with the rank this pivot rule gives, H · [s | G s] = 0, H is the input's columns
    taken by ``perm``; the built-in code is the packaged tables; alist files round-trip;
  * every limit raises a ValueError that names it;
  * the restated W-word sampler draws, for K <= 64, the one-word sampler's messages and classes;
  * the companion header binds beside the main one, whose interface is what it was, and both entry points validate before any launch;
  * ``LDPCModel()`` with its defaults is the model it was."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fgnn_oracle as O
import ldpc_code_oracle as CO
import ldpc_train_oracle as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANION = os.path.join(ROOT, 'include', 'fgnn_hip_ldpc_code.h')
NEW = ('fgnn_ldpc_encode_words', 'fgnn_ldpc_sample_rng_words')
EINVAL = -1                                    # FGNN_EINVAL
CODES = {'G12': (12, 3, 4, 0), 'G24': (24, 3, 6, 0), 'G132': (132, 3, 6, 0), 'G204': (204, 3, 6, 0)}
SIZES = {'G12': (9, 7, 5), 'G24': (12, 10, 14), 'G132': (66, 64, 68), 'G204': (102, 100, 104)}         # M, rank, K


def _gallager_h(n, dv, dc, seed):
    """The construction restated: band 0 consecutive, band b > 0 a permutation drawn in order."""
    rs = np.random.RandomState(seed)
    H = np.zeros((dv * n // dc, n), np.uint8)
    for b in range(dv):
        order = np.arange(n) if b == 0 else rs.permutation(n)
        for i, v in enumerate(order):
            H[b * (n // dc) + i // dc, v] = 1
    return H


@pytest.mark.parametrize('name', list(CODES))
def test_gallager_codes_are_regular_and_their_generator_fits(name):
    from fgnn_amd.ldpc_code import LdpcCode
    n, dv, dc, seed = CODES[name]
    c = CO.gallager(n, dv, dc, seed)
    M, rank, K = SIZES[name]
    assert (c.n_var, c.n_chk, c.dv, c.dc, c.P, c.K) == (n, M, dv, dc, rank, K) and c.K + c.P == c.n_var and not c.is_default
    assert c.H.shape == (M, n) and (c.H.sum(0) == dv).all() and (c.H.sum(1) == dc).all()
    assert c.G.shape == (c.P, c.K) and c.G.dtype == np.uint8 and c.W == -(-K // 64) and c.gwords.shape == (c.P, c.W)
    H0 = _gallager_h(n, dv, dc, seed)
    assert sorted(c.perm.tolist()) == list(range(n)) and np.array_equal(c.H, H0[:, c.perm])
    assert np.linalg.matrix_rank(H0.astype(np.float64)) >= rank                  # (over the reals: at least the GF(2) rank)
    s = np.random.RandomState(1).randint(0, 2, (64, c.K))
    cw = O.ldpc_encode(c.G, s)
    assert cw.shape == (64, n) and not ((cw.astype(np.int64) @ c.H.T.astype(np.int64)) % 2).any()
    # the tables are H's, lists increasing; nlist is what the sum-product oracle reads
    for v in range(n):
        assert c.var_to_factors[v].tolist() == np.nonzero(c.H[:, v])[0].tolist()
    for m in range(M):
        assert c.factor_to_vars[m].tolist() == np.nonzero(c.H[m])[0].tolist()
    assert np.array_equal(c.nlist, c.var_to_factors) and c.nlist.dtype == np.int32
    # packed rows: bit k of row r
    g = c.gwords
    assert all(int(g[r, k // 64] >> np.uint64(k % 64)) & 1 == c.G[r, k] for r in (0, c.P - 1) for k in range(c.K))
    # one code per (n, dv, dc, seed); immutable
    again = LdpcCode.gallager(n, dv, dc, seed)
    assert np.array_equal(again.G, c.G) and np.array_equal(again.perm, c.perm)
    assert not np.array_equal(LdpcCode.gallager(n, dv, dc, seed + 1).H, c.H)
    with pytest.raises(AttributeError):
        c.K = 3
    with pytest.raises(ValueError):
        c.G[0, 0] = 1


def test_builtin_is_the_packaged_code():
    from fgnn_amd.ldpc_code import LdpcCode
    from fgnn_amd.tables import _DATA, LdpcGraph
    c, g = LdpcCode.builtin(), LdpcGraph()
    z = np.load(os.path.join(_DATA, 'ldpc_96_3_963_G.npz'))
    assert (c.n_var, c.n_chk, c.dv, c.dc, c.K, c.P, c.W) == (96, 48, 3, 6, 48, 48, 1) and c.is_default
    assert np.array_equal(c.var_to_factors, g.var_to_factors) and np.array_equal(c.factor_to_vars, g.factor_to_vars)
    assert np.array_equal(c.nlist, z['A2_nlist']) and np.array_equal(c.G, z['G']) and np.array_equal(c.perm, np.arange(96))
    masks = (z['G'].astype(np.uint64) << np.arange(48, dtype=np.uint64)[None, :]).sum(1).astype(np.uint64)      # what LdpcDataPath packed
    assert np.array_equal(c.gwords[:, 0], masks)
    c.require_decoder().require_model()


def test_alist_round_trips(tmp_path):
    from fgnn_amd.ldpc_code import LdpcCode
    b = LdpcCode.builtin()
    p = str(tmp_path / 'builtin.alist')
    b.to_alist(p)
    lines = open(p).read().splitlines()
    assert lines[0].split() == ['96', '48'] and lines[1].split() == ['3', '6'] and len(lines) == 4 + 96 + 48
    assert [int(t) - 1 for t in lines[4].split()] == b.var_to_factors[0].tolist()
    back = LdpcCode.from_alist(p)
    assert np.array_equal(back.H, b.H[:, back.perm])                              # the same incidence, variables relabelled by perm
    assert not ((O.ldpc_encode(back.G, np.eye(back.K, dtype=np.int64)).astype(np.int64) @ back.H.T) % 2).any()
    c = CO.gallager(24, 3, 6, 0)
    q = str(tmp_path / 'g24.alist')
    c.to_alist(q)
    again = LdpcCode.from_alist(q)
    # the message positions already come first: the same pivots, no further relabelling, the same code
    assert np.array_equal(again.perm, np.arange(24)) and np.array_equal(again.H, c.H) and np.array_equal(again.G, c.G)
    assert np.array_equal(again.var_to_factors, c.var_to_factors) and np.array_equal(again.factor_to_vars, c.factor_to_vars)
    assert np.array_equal(LdpcCode.from_spec(q).G, c.G) and np.array_equal(LdpcCode.from_spec('gallager:24,3,6,0').G, c.G)
    assert LdpcCode.from_spec('builtin').is_default


def test_limits_and_malformed_codes_raise(tmp_path):
    from fgnn_amd.ldpc import LDPCModel
    from fgnn_amd.ldpc_code import LdpcCode
    H = CO.gallager(24, 3, 6, 0).H.copy()
    H[0, np.nonzero(H[0] == 0)[0][0]] = 1
    with pytest.raises(ValueError, match='irregular'):
        LdpcCode.from_parity_check(H)
    p = str(tmp_path / 'twice.alist')
    CO.gallager(12, 3, 4, 0).to_alist(p)
    lines = open(p).read().splitlines()
    first = lines[4].split()
    lines[4] = '\t'.join([first[0], first[0], first[2]])                          # variable 1 lists its first check twice
    open(p, 'w').write('\n'.join(lines) + '\n')
    with pytest.raises(ValueError, match='twice'):
        LdpcCode.from_alist(p)
    with pytest.raises(ValueError, match='multiple of dc'):
        LdpcCode.gallager(25, 3, 6, 0)
    with pytest.raises(ValueError, match='1025.*1024'):
        LdpcCode.gallager(1025, 3, 5, 0)
    with pytest.raises(ValueError, match='1025.*1024'):
        LdpcCode.from_parity_check(np.ones((1, 1025), np.uint8))
    big = LdpcCode.gallager(258, 3, 6, 0)                                         # fits the data path and the decoder, not the model
    assert big.require_decoder() is big
    with pytest.raises(ValueError, match='258.*132'):
        big.require_model()
    with pytest.raises(ValueError, match='258.*132'):
        LDPCModel.for_code(big)
    with pytest.raises(ValueError, match='258.*132'):
        LDPCModel(2, 6, 4, n_var=258, n_msg=100)
    with pytest.raises(ValueError, match='138.*132'):
        LDPCModel.for_code(LdpcCode.gallager(138, 3, 6, 0))                       # the model's limit is the verified size, not k <= 255
    g132 = CO.gallager(132, 3, 6, 0)
    assert g132.require_model() is g132 and LDPCModel.for_code(g132).n_var == 132
    # the training loop: the built-in code's shape class only, refused before any device work
    from fgnn_amd import ldpc_train
    for code, said in ((g132, 'N = 132'), (CO.gallager(12, 3, 4, 0), 'dc = 4'), (big, '258.*132')):
        with pytest.raises(ValueError, match=said):
            code.require_trainer()
        with pytest.raises(ValueError, match=said):
            ldpc_train.train(n_epochs=1, batch_size=8, steps_per_epoch=1, code=code, device='cuda')
    for ok in (CO.gallager(24, 3, 6, 0), CO.gallager(96, 3, 6, 0), LdpcCode.builtin()):
        assert ok.require_trainer() is ok
    wide = LdpcCode.gallager(344, 3, 8, 0)                                        # 1032 edges
    with pytest.raises(ValueError, match='1032.*1024'):
        wide.require_decoder()
    with pytest.raises(ValueError, match='gallager:N,dv,dc,seed'):
        LdpcCode.from_spec('gallager:24,3')


def test_restated_draws_are_the_one_word_samplers_for_k_up_to_64():
    """The restated W-word stream (tests/ldpc_code_oracle.py) against the one-word sampler's restatement (tests/ldpc_train_oracle.py) at
    the K of real codes, the word boundary included; and what the stream is for: batches that are codewords of an ``LdpcCode``."""
    from fgnn_amd import _hip
    from fgnn_amd.ldpc_code import LdpcCode
    assert 'fgnn_ldpc_sample_rng_words' in _hip.COMPANIONS and 'fgnn_ldpc_sample_rng' in _hip.COMPANIONS
    codes = [LdpcCode.builtin(), CO.gallager(12, 3, 4, 0), CO.gallager(24, 3, 6, 0)]
    assert [c.K for c in codes] == [48, 5, 14] and all(c.W == 1 for c in codes)
    for c in [CO.gallager(12, 3, 4, 0), CO.gallager(132, 3, 6, 0), CO.gallager(204, 3, 6, 0)]:
        cw, snr, sb, y = CO.sample_batch(c.G, 9, 5, 2)
        assert cw.shape == (9, c.n_var) and not ((cw.astype(np.int64) @ c.H.T.astype(np.int64)) % 2).any()
        assert np.array_equal(cw[:, :c.K], CO.sample_draws(9, 5, 2, c.K)[0]) and y.shape == cw.shape
    for K in [c.K for c in codes] + [1, 63, 64]:
        for seed, step in ((0, 0), (2 ** 64 - 59, 2 ** 33 + 1)):
            a = CO.sample_draws(70, seed, step, K)
            b = TR.sample_draws(70, seed, step, k=K)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (K, seed, step)
    # beyond one word: word 0 is the one-word sampler's, the further words come from blocks j >= 1 and the classes do not move
    s, i_snr, i_sigma = CO.sample_draws(70, 3, 9, 200)
    s64, j_snr, j_sigma = TR.sample_draws(70, 3, 9, k=64)
    assert np.array_equal(s[:, :64], s64) and np.array_equal(i_snr, j_snr) and np.array_equal(i_sigma, j_sigma)
    assert 0.4 < s[:, 64:].mean() < 0.6 and len({s[:, 64 * w:64 * w + 8].tobytes() for w in range(3)}) == 3
    short = CO.sample_draws(70, 3, 9, 130)[0]
    assert np.array_equal(short, s[:, :130])                                      # K only cuts the stream


def test_checkpoint_entry_names_the_code():
    from fgnn_amd.ldpc_code import LdpcCode
    c, b = CO.gallager(24, 3, 6, 0), LdpcCode.builtin()
    e = c.checkpoint_entry()
    assert set(e) == {'n_var', 'n_chk', 'dv', 'dc', 'var_to_factors'} and all(isinstance(v, torch.Tensor) for v in e.values())
    assert [int(e[k]) for k in ('n_var', 'n_chk', 'dv', 'dc')] == [24, 12, 3, 6]
    assert torch.equal(e['var_to_factors'], torch.from_numpy(c.var_to_factors.copy()))
    c.check_checkpoint({'code': e})
    b.check_checkpoint({})                                                        # no entry: the default code's
    with pytest.raises(ValueError, match='trained for a code with') as err:
        b.check_checkpoint({'code': e})
    assert 'another incidence' not in str(err.value)                              # other sizes: nothing to add
    with pytest.raises(ValueError, match='built-in 96.3.963') as err:
        c.check_checkpoint({})
    assert 'another incidence' not in str(err.value)
    with pytest.raises(ValueError, match='same sizes but another incidence'):
        LdpcCode.gallager(24, 3, 6, 1).check_checkpoint({'code': e})


def test_companion_header_is_parsed_bound_and_built():
    from fgnn_amd import _hip
    text = open(COMPANION).read()
    assert '#include "fgnn_hip.h"' in text and 'extern "C"' in text
    sig = _hip.signatures(text)
    assert tuple(sig) == NEW == _hip.LDPC_CODE
    assert not set(NEW) & set(_hip.EXPORTS) and not set(NEW) & set(_hip.SIGNATURES)
    assert _hip.ABI_VERSION == 15 and len(_hip.EXPORTS) == len(_hip.SIGNATURES) == 90
    main = open(_hip.HEADER_PATH).read()
    assert not any(re.search(r'\b%s\b' % name, main) for name in NEW)
    L = _hip.lib()
    for name in NEW:
        fn = getattr(L, name)                                        # exported by the built library ...
        restype, params = sig[name]
        assert fn.restype is restype is ctypes.c_int32               # ... and bound with the parsed types
        assert list(fn.argtypes) == [t for _, t in params] and _hip.COMPANIONS[name][:2] == sig[name]
    assert [n for n, _ in sig[NEW[0]][1]] == ['s', 'gwords', 'B', 'K', 'P', 'W', 'cw', 'stream']
    old = [n for n, _ in _hip.COMPANIONS['fgnn_ldpc_sample_rng'][1]]
    want = [('gwords' if n == 'gmask' else n) for n in old]
    want.insert(want.index('P') + 1, 'W')
    assert [n for n, _ in sig[NEW[1]][1]] == want                    # the one-word sampler's arguments, gwords for gmask, W behind P
    args = dict(sig[NEW[1]][1])
    assert args['seed'] is ctypes.c_uint64 and args['B'] is ctypes.c_int64 and args['W'] is ctypes.c_int32
    assert args['gwords'] is _hip.DevicePointer and args['stream'] is _hip.DevicePointer


def test_entry_points_validate_before_any_launch():
    from fgnn_amd import _hip
    L = _hip.lib()
    one = ctypes.c_void_p(16)                      # a non-NULL pointer that is never dereferenced on these paths
    enc = lambda s=one, g=one, B=4, K=100, P=60, W=2, cw=one: _hip.invoke('fgnn_ldpc_encode_words', s, g, B, K, P, W, cw, None)
    assert enc(s=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert enc(g=None) == EINVAL and enc(cw=None) == EINVAL and enc(B=-1) == EINVAL
    assert enc(K=1000, P=25, W=16) == _hip.EUNSUPPORTED and b'1024' in L.fgnn_last_error()
    assert enc(K=0, W=0) == _hip.EUNSUPPORTED and enc(P=-1) == _hip.EUNSUPPORTED
    for K, W in ((100, 1), (100, 3), (64, 2), (65, 1), (128, 3)):
        assert enc(K=K, W=W) == _hip.EUNSUPPORTED and b'ceil(K / 64)' in L.fgnn_last_error(), (K, W)
    assert enc(s=None, g=None, cw=None, B=0) == 0                                  # empty batch: nothing to do
    assert enc(K=1025, P=0, W=17, B=0) == _hip.EUNSUPPORTED                        # ... but the sizes are still checked
    f2 = (ctypes.c_float * 2)(0.0, 1.0)

    def smp(B=4, K=100, P=60, W=2, n_snr=2, n_sigma=2, dtype=None, nchk=80, node=one, g=one, snr=f2):
        return _hip.invoke('fgnn_ldpc_sample_rng_words', 0, 0, snr, n_snr, f2, n_sigma, 0.05, g, one, one, B, K, P, W, nchk, 3, 6,
                           _hip.F32 if dtype is None else dtype, node, one, one, one, one, one, None, None, None, None)
    assert smp(node=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert smp(g=None) == EINVAL and smp(snr=None) == EINVAL
    assert smp(B=-1) == EINVAL and smp(n_snr=0) == EINVAL and smp(n_sigma=0) == EINVAL
    assert smp(K=1000, P=25, W=16) == _hip.EUNSUPPORTED and b'1024' in L.fgnn_last_error()
    assert smp(W=1) == _hip.EUNSUPPORTED and b'ceil(K / 64)' in L.fgnn_last_error()
    assert smp(P=0) == _hip.EUNSUPPORTED and smp(K=0, W=0) == _hip.EUNSUPPORTED and smp(nchk=0) == _hip.EUNSUPPORTED
    assert smp(n_snr=17) == _hip.EUNSUPPORTED and smp(dtype=7) == _hip.EUNSUPPORTED and smp(B=2 ** 31) == _hip.EUNSUPPORTED
    assert smp(node=None, g=None, B=0) == 0


def test_default_model_is_the_model_it_was():
    from fgnn_amd.ldpc import LDPCModel
    old, new = LDPCModel(2, 6, 4).state_dict(), LDPCModel(2, 6, 4, n_var=96, n_msg=48).state_dict()
    assert len(old) == 651 and list(old) == list(new)
    assert all(old[k].shape == new[k].shape and old[k].dtype == new[k].dtype for k in old)
    assert old['emodel_f2v.0.weight'].shape[1] == 7 and old['hnn_idx_v2f'].shape == (1, 1, 96)
    c = CO.gallager(24, 3, 6, 0)
    m = LDPCModel.for_code(c)
    sd = m.state_dict()
    assert (m.n_var, m.n_msg) == (24, 14) and list(sd) == list(old)                # the same entries, shapes by the code
    assert sd['hnn_idx_v2f'].shape == (1, 1, 24) and sd['hetype_f2v'].shape == (1, 1, 24, 1) and sd['emodel_v2f.0.weight'].shape[1] == 7
    m4 = LDPCModel.for_code(CO.gallager(12, 3, 4, 0))
    assert m4.state_dict()['emodel_f2v.0.weight'].shape[1] == 5                   # dc + 1 raw edge features


def test_host_layers_take_a_code_without_a_device():
    from fgnn_amd import ldpc_eval, ldpc_train
    from fgnn_amd.datapath import LdpcDataPath, check_received_args
    c = CO.gallager(132, 3, 6, 0)                                                 # within the model's limit, beyond the trainer's
    y = torch.zeros(3, 132)
    assert check_received_args(y, torch.zeros(3), torch.float32, 132) == 3 and check_received_args(y, torch.zeros(3, 132), torch.float32, 132) == 3
    assert check_received_args(torch.zeros(3, 96), torch.zeros(3, 96), torch.float32) == 3          # the default is the built-in code's
    with pytest.raises(ValueError, match=r'\[B, 132\]'):
        check_received_args(torch.zeros(3, 96), torch.zeros(3), torch.float32, 132)
    with pytest.raises(ValueError, match=r'\[B, 96\]'):
        check_received_args(y, torch.zeros(3), torch.float32)
    ts = {'noizy_sg': y, 'gts': torch.zeros(3, 132, dtype=torch.int64), 'snr_dbs': torch.zeros(3, 132), 'sigma_b': torch.zeros(3)}
    assert ldpc_eval.load_test_set(ts, 'cpu', 132)[0].shape == (3, 132)
    with pytest.raises(ValueError, match=r'n,96'):
        ldpc_eval.load_test_set(ts, 'cpu')
    with pytest.raises(RuntimeError, match='ROCm device'):
        LdpcDataPath('cpu', c)
    m = ldpc_train.build_model('max', c)
    assert (m.n_var, m.n_msg) == (132, 68) and ldpc_train.build_model('max').n_var == 96
    opt = torch.optim.Adam(m.parameters())
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=ldpc_train.lr_sched)
    ck = ldpc_train.checkpoint_dict(m, opt, sched, 1, 2, c)
    assert set(ck) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt', 'code'}
    from fgnn_amd.ldpc_code import LdpcCode
    for default in (None, LdpcCode.builtin()):                                    # the default code's dict is the script's
        assert set(ldpc_train.checkpoint_dict(m, opt, sched, 1, 2, default)) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt'}
    with pytest.raises(ValueError, match='K = 48 of N = 96'):
        ldpc_eval.evaluate(m, ts)                                                 # a model of another code, before any device work


@pytest.mark.parametrize('name', ('g12', 'builtin', 'g32', 'g384', 'g1024'))
def test_incidence_tables_are_the_restatements(name):
    import ldpc_llr_oracle as LO
    import test_ldpc_llr_gpu as G
    assert G.CODES == ('g12', 'builtin', 'g32', 'g384', 'g1024')
    code = G.case(name)[0]
    got, want = code.incidence_tables(), LO.tables(code.nlist, code.n_chk)
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert isinstance(a, np.ndarray) and a.dtype == np.int32 and not a.flags.writeable
        assert a.shape == np.shape(b) and np.array_equal(a, b)
    assert all(a is b for a, b in zip(code.incidence_tables(), got))          # memoised
