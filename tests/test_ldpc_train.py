"""Host side of the LDPC trainer (fgnn_amd/ldpc_train.py): the companion header and its binding, the two new entry points' argument
checks, the schedule arithmetic, the checkpoint layout, the input checks of decoding_loss_parts / sample_rng, and the statistics of
the sampler's restated draws (tests/ldpc_train_oracle.py).  No GPU needed."""
import contextlib
import ctypes
import io
import math
import os
import re

import numpy as np
import pytest
import torch

import ldpc_train_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPANION = os.path.join(ROOT, 'include', 'fgnn_hip_ldpc_train.h')
NEW = ('fgnn_ldpc_sample_rng', 'fgnn_ldpc_loss_parts_forward')
EINVAL = -1


def test_companion_header_is_parsed_bound_and_built():
    from fgnn_amd import _hip
    text = open(COMPANION).read()
    assert '#include "fgnn_hip.h"' in text and 'extern "C"' in text
    sig = _hip.signatures(text)
    assert tuple(sig) == NEW == _hip.LDPC_TRAIN
    # the main header's interface is what it was: the companion's names are not among its exports
    assert not set(NEW) & set(_hip.EXPORTS) and not set(NEW) & set(_hip.SIGNATURES) and _hip.ABI_VERSION == 15
    main = open(_hip.HEADER_PATH).read()
    assert not any(re.search(r'\b%s\b' % name, main) for name in NEW)
    L = _hip.lib()
    for name in NEW:
        fn = getattr(L, name)                                        # exported by the built library ...
        restype, params = sig[name]
        assert fn.restype is restype is ctypes.c_int32               # ... and bound with the parsed types
        assert list(fn.argtypes) == [t for _, t in params] and _hip.COMPANIONS[name][:2] == sig[name]
    args = dict(sig['fgnn_ldpc_sample_rng'][1])
    assert args['seed'] is ctypes.c_uint64 and args['offset'] is ctypes.c_uint64 and args['B'] is ctypes.c_int64
    assert args['rho'] is ctypes.c_float and args['snr_choices'] is _hip.DevicePointer and args['stream'] is _hip.DevicePointer
    assert [n for n, _ in sig['fgnn_ldpc_loss_parts_forward'][1]] == [
        'logits', 'label', 'pred', 'sigma_b', 'B', 'n', 'dtype', 'mse_weight', 'out', 'counts', 'workspace', 'workspace_bytes', 'stream']
    # each entry point cites the reference lines it replaces
    assert 'ldpc_dataset.py:222-236' in text and 'lib/data/ldpc.py:7-30' in text and 'train_ldpc.py:232-251' in text


def _sample(**kw):
    """fgnn_ldpc_sample_rng through ``_hip.invoke`` with never-dereferenced pointers (every check runs before any launch)."""
    from fgnn_amd import _hip
    p = ctypes.c_void_p(4096)
    five, six = (ctypes.c_float * 17)(*range(17)), (ctypes.c_float * 17)(*range(17))
    a = dict(seed=0, offset=0, snr_choices=five, n_snr=5, sigma_choices=six, n_sigma=6, rho=0.05, gmask=p, var_to_factors=p,
             factor_to_vars=p, B=4, K=48, P=48, nchk=48, dv=3, dc=6, dtype=_hip.F32, node=p, hop=p, ef_f2v=p, ef_v2f=p, snr_db=p,
             sigma_b=p, cw=None, label=None, y=None, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return _hip.invoke('fgnn_ldpc_sample_rng', *a.values())


def test_sampler_validates_its_arguments_without_a_gpu():
    from fgnn_amd import _hip
    L = _hip.lib()
    for name in ('snr_choices', 'sigma_choices', 'gmask', 'var_to_factors', 'factor_to_vars', 'node', 'hop', 'ef_f2v', 'ef_v2f', 'snr_db',
                 'sigma_b'):
        assert _sample(**{name: None}) == EINVAL and b'null' in L.fgnn_last_error(), name
    assert _sample(K=65) == _hip.EUNSUPPORTED and b'K=65' in L.fgnn_last_error()
    assert _sample(P=65) == _hip.EUNSUPPORTED and _sample(K=0) == _hip.EUNSUPPORTED
    assert _sample(dv=0) == _hip.EUNSUPPORTED and _sample(dc=0) == _hip.EUNSUPPORTED and _sample(nchk=0) == _hip.EUNSUPPORTED
    assert _sample(n_snr=0) == EINVAL and _sample(n_sigma=0) == EINVAL and _sample(n_snr=-3) == EINVAL
    assert _sample(n_snr=17) == _hip.EUNSUPPORTED and _sample(n_sigma=17) == _hip.EUNSUPPORTED
    assert _sample(n_snr=16, n_sigma=16, B=0) == 0
    assert _sample(dtype=2) == _hip.EUNSUPPORTED
    assert _sample(B=-1) == EINVAL
    assert _sample(B=0) == 0 and _sample(B=0, node=None, gmask=None) == 0        # an empty batch: nothing to do
    with pytest.raises(TypeError, match='fgnn_ldpc_sample_rng takes 27 arguments'):
        _hip.invoke('fgnn_ldpc_sample_rng', 0, 0)


def test_loss_parts_validates_its_arguments_without_a_gpu():
    from fgnn_amd import _hip
    L = _hip.lib()
    p = ctypes.c_void_p(4096)
    ws = int(L.fgnn_ldpc_loss_workspace_bytes())

    def parts(logits=p, label=p, pred=p, sigma_b=p, B=4, n=48, dtype=_hip.F32, out=p, counts=None, w=p, wb=ws):
        return _hip.invoke('fgnn_ldpc_loss_parts_forward', logits, label, pred, sigma_b, B, n, dtype, 0.1, out, counts, w, wb, None)

    for name in ('logits', 'label', 'pred', 'sigma_b', 'out', 'w'):
        assert parts(**{name: None}) == EINVAL, name
    assert b'workspace' in L.fgnn_last_error()
    assert parts(wb=ws - 8) == EINVAL and b'workspace' in L.fgnn_last_error()
    assert parts(w=ctypes.c_void_p(4100)) == EINVAL and parts(counts=ctypes.c_void_p(4100)) == EINVAL
    assert parts(B=0) == EINVAL and parts(n=0) == EINVAL and parts(dtype=2) == EINVAL
    # the plain forward checks the same things (one launcher under both)
    assert L.fgnn_ldpc_loss_forward(p, p, p, p, 4, 48, 0, 0.1, p, p, ws - 8, None) == EINVAL
    assert L.fgnn_ldpc_loss_forward(p, p, p, p, 4, 48, 0, 0.1, None, p, ws, None) == EINVAL


def test_a_library_without_a_companion_symbol_says_rebuild(tmp_path):
    """``bind_header`` on a header whose entry point the built library does not have: the library still loads and serves every other
    name; calling the missing one raises FgnnHipError (not AttributeError) that says to rebuild."""
    from fgnn_amd import _hip
    h = tmp_path / 'fgnn_hip_later.h'
    h.write_text('#include "fgnn_hip.h"\nextern "C" {\n/* fgnn_in_a_comment(int x); */\nint fgnn_not_built_yet(const float* x, '
                 'int64_t n, fgnn_stream_t stream);\n}\n')
    before = (_hip.SIGNATURES, _hip.EXPORTS)
    try:
        assert _hip.bind_header(str(h)) == ('fgnn_not_built_yet',)
        assert (_hip.SIGNATURES, _hip.EXPORTS) == before and 'fgnn_not_built_yet' not in _hip.EXPORTS
        with pytest.raises(TypeError, match='takes 3 arguments'):            # the count check (stream defaulting included) holds here too
            _hip.invoke('fgnn_not_built_yet', None)
        with pytest.raises(_hip.FgnnHipError, match='rebuild'):
            _hip.invoke('fgnn_not_built_yet', None, 0, None)
        with pytest.raises(_hip.FgnnHipError, match='rebuild'):
            _hip.call('fgnn_not_built_yet', None, 0, None)
        assert _hip.lib().fgnn_abi_version() == 15
    finally:
        _hip.COMPANIONS.pop('fgnn_not_built_yet', None)
        _hip._MISSING.pop('fgnn_not_built_yet', None)
    with pytest.raises(KeyError):                                          # in neither table: as before companions existed
        _hip.invoke('fgnn_not_built_yet', None, 0, None)
    again = tmp_path / 'again.h'
    again.write_text('int fgnn_ldpc_encode(int32_t n);\n')
    with pytest.raises(_hip.FgnnHipError, match='again'):                   # a companion may not redeclare a main-header name
        _hip.bind_header(str(again))
    with pytest.raises(_hip.FgnnHipError, match='no_such.h'):
        _hip.bind_header('no_such.h')


def test_schedule_matches_lambda_lr_stepped_as_the_script_steps_it():
    """train_ldpc.py:163-169,253: scheduler.step() at the END of every epoch.  Epoch e trains at 1e-2 * lr_sched(e)."""
    from fgnn_amd import ldpc_train as T

    def script_lr_sched(x, start=10):
        if x <= start:
            return max(1e-2, (1.0 / start) * x)
        else:
            return max(0.99 ** (x - start), 1e-6)

    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-2, weight_decay=1e-8)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: script_lr_sched(x))
    for e in range(26):
        assert T.lr_sched(e) == script_lr_sched(e)
        assert opt.param_groups[0]['lr'] == T.epoch_lr(e) == 1e-2 * script_lr_sched(e), e
        opt.step()
        sched.step()
    assert T.epoch_lr(0) == 1e-4 and T.epoch_lr(10) == 1e-2 and T.epoch_lr(12) == 1e-2 * 0.99 ** 2 and T.epoch_lr(0, 1e-1) == 1e-3
    assert T.lr_sched(10 ** 5) == 1e-6
    assert T.default_steps_per_epoch(32) == math.ceil(10000 / 32) == 313
    assert T.default_steps_per_epoch(4096) == 3 and T.default_steps_per_epoch(10000) == 1 and T.default_steps_per_epoch(10001) == 1
    with pytest.raises(ValueError):
        T.default_steps_per_epoch(0)


def test_checkpoint_is_the_scripts_and_a_stock_adam_loads_it(tmp_path):
    """The script's path and dict keys; a FastAdam-written ``optimizer_state_dict`` (after a step, on the CPU) loads into
    ``torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=1e-8)`` composed as the script composes it, and the model state loads
    strictly into a fresh LDPCModel."""
    from fgnn_amd import ldpc_train as T
    from fgnn_amd.fastpath import FastAdam
    assert T.checkpoint_path('out', 'FactorNN', 10, None) == os.path.join('out', 'FactorNN_nn_factor_epoches_10_snr_None.pt')
    assert T.checkpoint_path('.', 'm', 3, 2) == os.path.join('.', 'm_nn_factor_epoches_3_snr_2.pt')
    torch.manual_seed(0)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        model = T.build_model('max')
    assert out.getvalue() == ''                                      # the construction's talk goes to stderr
    opt = FastAdam(model.parameters(), lr=T.LR, weight_decay=T.WEIGHT_DECAY)
    sched = T._scheduler(opt)
    for q in model.parameters():
        if q.requires_grad:
            q.grad.fill_(1e-3)
    opt.step()
    sched.step()
    d = T.checkpoint_dict(model, opt, sched, 1, 7)
    assert set(d) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt'} and d['epoch'] == 1 and d['gcnt'] == 7
    path = str(tmp_path / 'c.pt')
    torch.save(d, path)
    back = torch.load(path, map_location='cpu', weights_only=True)
    with contextlib.redirect_stdout(io.StringIO()):
        fresh = T.build_model('max')
    fresh.load_state_dict(back['model_state_dict'], strict=True)
    stock = torch.optim.Adam(fresh.parameters(), lr=1e-2, weight_decay=1e-8)
    sched2 = torch.optim.lr_scheduler.LambdaLR(stock, lr_lambda=lambda x: T.lr_sched(x))
    stock.load_state_dict(back['optimizer_state_dict'])
    sched2.load_state_dict(back['lr_sche'])
    assert sched2.last_epoch == 1 and stock.param_groups[0]['lr'] == T.epoch_lr(1) and stock.param_groups[0]['weight_decay'] == 1e-8
    assert len(stock.param_groups[0]['params']) == len(list(fresh.parameters()))
    assert back['optimizer_state_dict']['state'] and all(int(st['step']) == 1 for st in back['optimizer_state_dict']['state'].values())


def test_host_side_refusals():
    from fgnn_amd import ldpc_train as T
    from fgnn_amd.datapath import LdpcDataPath, check_sample_rng_args
    from fgnn_amd.ldpc import decoding_loss_parts
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        T.train(device='cpu')
    with pytest.raises(ValueError):
        T.train(n_epochs=1, batch_size=0, device='cpu')
    with pytest.raises(ValueError):
        T.train(n_epochs=1, dtype=torch.float16, device='cpu')
    with pytest.raises(RuntimeError):
        LdpcDataPath('cpu')
    ok = dict(B=4, seed=0, step=0, dtype=torch.float32, choices_snr=(0, 1), choices_sigma=(0,), out=None)
    check_sample_rng_args(**ok)
    for bad in (dict(B=-1), dict(seed=2 ** 64), dict(seed=-1), dict(step=2 ** 63), dict(step=-1), dict(dtype=torch.float16),
                dict(choices_snr=()), dict(choices_snr=tuple(range(17))), dict(choices_sigma=(float('nan'),)), dict(out=(1, 2))):
        with pytest.raises(ValueError):
            check_sample_rng_args(**dict(ok, **bad))
    logits, pred, label, sb = torch.zeros(4, 48), torch.zeros(4, 1), torch.zeros(4, 48), torch.zeros(4)
    bad = [(logits[0], pred, label, sb), (logits.double(), pred, label, sb), (logits.half(), pred, label, sb),
           (logits, pred.double(), label, sb), (logits, torch.zeros(5, 1), label, sb), (logits, torch.zeros(4, 2), label, sb),
           (logits, pred, label[:, :47], sb), (logits, pred, label, torch.zeros(3)), (torch.zeros(0, 48), torch.zeros(0, 1), torch.zeros(0, 48), torch.zeros(0))]
    for args in bad:
        with pytest.raises(ValueError):
            decoding_loss_parts(*args)
    for counts in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int64)[::2]):
        with pytest.raises(ValueError):
            decoding_loss_parts(logits, pred, label, sb, counts=counts)
    with pytest.raises(RuntimeError, match='no CPU fallback'):       # well-formed, but not on a ROCm device
        decoding_loss_parts(logits, pred, label, sb, counts=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        decoding_loss_parts(logits.bfloat16(), pred[:, 0], label, sb)


@pytest.mark.parametrize('seed, step', [(0, 0), (7, 3)])
def test_restated_draws_are_uniform_and_distinct(seed, step):
    """60000 codewords of the restatement: every frequency within 5 binomial standard deviations of its expectation — sqrt(p (1 - p)
    / 60000) x 5 = 0.0082 for p = 1/5, 0.0076 for 1/6, 0.0037 for 1/30, 0.0102 for 1/2 — and no message drawn twice (2^48 messages:
    a collision among 60000 has probability 6e-6)."""
    n = 60000
    s, i_snr, i_sigma = R.sample_draws(n, seed, step)
    assert s.shape == (n, 48) and set(np.unique(s)) == {0, 1}
    f_snr = np.bincount(i_snr, minlength=5) / n
    f_sigma = np.bincount(i_sigma, minlength=6) / n
    joint = np.bincount(i_snr * 6 + i_sigma, minlength=30) / n
    bits = s.mean(0)
    print('snr', f_snr, 'sigma', f_sigma, 'joint max dev', np.abs(joint - 1 / 30).max(), 'bit max dev', np.abs(bits - 0.5).max())
    assert len(f_snr) == 5 and len(f_sigma) == 6 and len(joint) == 30
    assert np.abs(f_snr - 1 / 5).max() <= 0.0082
    assert np.abs(f_sigma - 1 / 6).max() <= 0.0076
    assert np.abs(joint - 1 / 30).max() <= 0.0037
    assert np.abs(bits - 0.5).max() <= 0.0102
    packed = (s.astype(np.uint64) << np.arange(48, dtype=np.uint64)[None, :]).sum(1)
    assert len(np.unique(packed)) == n
    # another step, other messages; the same (seed, step), the same
    s2 = R.sample_draws(64, seed, step + 1)[0]
    assert not np.array_equal(s2, s[:64]) and np.array_equal(R.sample_draws(64, seed, step)[0], s[:64])


def test_restated_draws_against_plain_integer_arithmetic():
    """The restatement's bit and class-index arithmetic (numpy uint64 shifts and products) against the header's rule written with
    Python integers, word by word, on Philox blocks formed one at a time — at a seed and step that use all 64 bits, and at the
    extreme words 0 and 2^32 - 1 (class 0 and class n - 1)."""
    import fgnn_oracle as O
    seed, step = 0x1234567887654321, 2 ** 33 + 5
    s, i_snr, i_sigma = R.sample_draws(40, seed, step, n_snr=5, n_sigma=6)
    for b in (0, 1, 17, 39):
        r = [int(v) for v in O.philox4x32(np.array([b, 0x80000000, step & 0xFFFFFFFF, step >> 32], np.uint64),
                                          (seed & 0xFFFFFFFF, seed >> 32))]
        bits = [(r[0] >> c) & 1 if c < 32 else (r[1] >> (c - 32)) & 1 for c in range(48)]
        assert s[b].tolist() == bits
        assert int(i_snr[b]) == (r[2] * 5) >> 32 and int(i_sigma[b]) == (r[3] * 6) >> 32
        assert 0 <= int(i_snr[b]) < 5 and 0 <= int(i_sigma[b]) < 6
    for n in (1, 5, 6, 16):
        assert (0 * n) >> 32 == 0 and ((2 ** 32 - 1) * n) >> 32 == n - 1
    # 64 message bits (K = 64): word 1's top bit is message bit 63
    s64 = R.sample_draws(3, seed, step, k=64)[0]
    r = [int(v) for v in O.philox4x32(np.array([2, 0x80000000, step & 0xFFFFFFFF, step >> 32], np.uint64), (seed & 0xFFFFFFFF, seed >> 32))]
    assert s64[2].tolist() == [((r[0] | (r[1] << 32)) >> c) & 1 for c in range(64)]
