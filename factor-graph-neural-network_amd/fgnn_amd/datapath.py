"""The LDPC data path in front of the decoder, per batch on the GPU: the encoder, the channel, the model's
features, the batch samplers and the test-set writers.  The classical decoders a path also runs live in ``ldpc_decoders``.

The reference builds every training item on the host: ``gen_data_item`` (/root/reference/lib/data/ldpc.py:7-30)
calls the pybind11 MNC library for the GF(2) encode ``s2t`` and the channel ``t2y``
(lib/data/MNC/MNC_py.cpp:22-108), then ``ContinousCodesSP.__getitem__``
(lib/data/ldpc_dataset.py:222-236) assembles the model inputs with numpy takes.  ``LdpcDataPath`` produces a whole
batch of the same eight arrays with two kernels (csrc/ldpc_datapath.hip) in the dtype the model kernels read.
No CPU fallback: the arrays are produced where they are consumed.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _hip
from .ldpc_code import LdpcCode
from .ldpc_decoders import LdpcDecoders, parse_decoder


# ``LdpcDataPath.sample_rng``'s result: the reference's DataLoader item (train_ldpc.py:207) in its order, then what the sampler drew
# besides — the SNR per word, the whole codeword (uint8) and the received word
LdpcBatch = collections.namedtuple('LdpcBatch', 'node_feature hop_feature nn_idx_f2v nn_idx_v2f efeature_f2v efeature_v2f label sigma_b '
                                                'snr_db cw y')


def check_sample_rng_args(B, seed, step, dtype, choices_snr, choices_sigma, out):
    """Arguments of ``LdpcDataPath.sample_rng`` (before anything reaches the device)."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('dtype must be float32 or bfloat16')
    if int(B) < 0:
        raise ValueError('B must be >= 0, got %d' % B)
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError('seed must fit 64 bits')
    if not 0 <= int(step) < 2 ** 63:
        raise ValueError('step must be in [0, 2^63): bit 63 of the offset selects the channel kernel\'s second stream')
    for what, c in (('snr_db', choices_snr), ('sigma_b', choices_sigma)):
        if not 1 <= len(c) <= 16 or any(not np.isfinite(float(v)) for v in c):
            raise ValueError('%s choices: 1 to 16 finite values, got %s' % (what, tuple(c)))
    if out is not None:
        if not isinstance(out, LdpcBatch) or out.node_feature.shape[0] != int(B) or out.node_feature.dtype != dtype:
            raise ValueError('out must be a previous sample_rng result for the same (B, dtype)')


class LdpcDataPath(LdpcDecoders):
    """The data path of one regular LDPC code (``code``: an ``LdpcCode``; None: the built-in 96.3.963 — 48 message bits, 48 parity
    bits, 3 checks per variable, 6 variables per check): K message bits, P parity bits (codeword = [s | G s]), N = K + P variables,
    M checks.  The shapes below are written for the built-in code; for another, 96 reads N, 48 reads K (bits) or M (checks), 3 reads
    dv and 6 / 7 read dc / dc + 1.  A code whose rows of G fit one 64-bit word (K, P <= 64) runs the one-word encoder and sampler
    (csrc/ldpc_datapath.hip), as the built-in code always has; any other the W-word ones (csrc/ldpc_code.hip).
    ``sample`` mirrors ``ContinousCodesSP.__getitem__`` over a batch.  The decoders (``decode``, ``decode_llr``, ``decode_osd``) are
    the base class's (``ldpc_decoders.LdpcDecoders``)."""
    K, P = 48, 48                                   # (the built-in code's; an instance carries its code's)
    sigma_b_choices = (0, 1, 2, 3, 4, 5)            # ldpc_dataset.py:212
    snr_db_choices = (0, 1, 2, 3, 4)                # ldpc_dataset.py:216

    def __init__(self, device, code=None):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('LdpcDataPath runs on a ROCm device (no CPU fallback)')
        code = LdpcCode.builtin() if code is None else code
        if not isinstance(code, LdpcCode):
            raise TypeError('code must be an LdpcCode or None, got %s' % type(code).__name__)
        self.code = code
        self.K, self.P, self.N, self.M, self.dv, self.dc, self.W = code.K, code.P, code.n_var, code.n_chk, code.dv, code.dc, code.W
        self.one_word = code.K <= 64 and 1 <= code.P <= 64       # the one-word kernels' family (fgnn_ldpc_encode, fgnn_ldpc_sample_rng)
        super().__init__()                                       # the decoders' state: device tables, loaded learned checkpoints
        gwords = code.gwords.view(np.int64)                       # [P, W]; the one-word kernels' gmask is its column 0, [P]
        self.gmask = torch.from_numpy((gwords[:, 0] if self.one_word else gwords).copy()).to(self.device)
        self.var_to_factors = torch.from_numpy(code.var_to_factors.astype(np.int32)).to(self.device)
        self.factor_to_vars = torch.from_numpy(code.factor_to_vars.astype(np.int32)).to(self.device)
        self.nn_idx_f2v = torch.from_numpy(code.var_to_factors.copy()).to(self.device)
        self.nn_idx_v2f = torch.from_numpy(code.factor_to_vars.copy()).to(self.device)

    def _features(self, B, dtype):
        """Empty (node_feature, hop_feature, efeature_f2v, efeature_v2f) for B words."""
        new = lambda *shape: torch.empty(shape, device=self.device, dtype=dtype)
        return (new(B, 2, self.N, 1), new(B, self.dc, self.M, 1), new(B, self.dc + 1, self.N, self.dv),
                new(B, self.dc + 1, self.M, self.dc))

    def encode(self, s):
        """s [B,48] (any integer / bool dtype, values 0/1) -> codewords [B,96] uint8 = [s | G s mod 2]."""
        if s.dim() != 2 or s.shape[1] != self.K:
            raise ValueError('messages must be [B, %d], got %s' % (self.K, tuple(s.shape)))
        s = s.to(self.device, torch.uint8).contiguous()
        B = s.shape[0]
        cw = torch.empty((B, self.K + self.P), device=self.device, dtype=torch.uint8)
        if self.one_word:
            _hip.call('fgnn_ldpc_encode', s, self.gmask, B, self.K, self.P, cw)
        else:
            _hip.call('fgnn_ldpc_encode_words', s, self.gmask, B, self.K, self.P, self.W, cw)
        return cw

    def channel_features(self, cw, snr_db, sigma_b, burst_prob=0.05, noise=None, generator=None,
                         dtype=torch.float32, kernel_rng=None):
        """Received words + model inputs for codewords cw [B,96].  ``noise`` = (z1, u, z2) [B,96] f32 draws
        (standard normal, uniform [0,1), standard normal); drawn from ``generator`` when None.  ``kernel_rng`` = (seed,
        offset): no noise tensors at all — the kernel draws them itself (Philox4x32-10 keyed by seed, counter = (bit index,
        offset); csrc/ldpc_datapath.hip, restated in oracle/fgnn_oracle.py::philox_channel_draws).
        Returns (y [B,96] f32, node_feature [B,2,96,1], hop_feature [B,6,48,1], efeature_f2v [B,7,96,3],
        efeature_v2f [B,7,48,6])."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('dtype must be float32 or bfloat16')
        if cw.dim() != 2 or cw.shape[1] != self.N:
            raise ValueError('codewords must be [B, %d], got %s' % (self.N, tuple(cw.shape)))
        B, N = cw.shape
        dev = self.device
        cw = cw.to(dev, torch.uint8).contiguous()
        snr_db = snr_db.to(dev, torch.float32).contiguous()
        sigma_b = sigma_b.to(dev, torch.float32).contiguous()
        if kernel_rng is not None:
            z1 = u = z2 = None
        elif noise is None:
            z1 = torch.randn((B, N), device=dev, generator=generator)
            u = torch.rand((B, N), device=dev, generator=generator)
            z2 = torch.randn((B, N), device=dev, generator=generator)
        else:
            z1, u, z2 = [t.to(dev, torch.float32).contiguous() for t in noise]
        y = torch.empty((B, N), device=dev, dtype=torch.float32)
        node, hop, ef_f2v, ef_v2f = self._features(B, dtype)
        if kernel_rng is not None:
            seed, offset = (int(v) & 0xFFFFFFFFFFFFFFFF for v in kernel_rng)
            _hip.call('fgnn_ldpc_channel_features_rng', cw, snr_db, sigma_b, float(burst_prob), seed, offset, self.var_to_factors,
                      self.factor_to_vars, B, self.N, self.M, self.dv, self.dc, _hip.dtype_code(node), y, node, hop, ef_f2v, ef_v2f)
            return y, node, hop, ef_f2v, ef_v2f
        _hip.call('fgnn_ldpc_channel_features', cw, snr_db, sigma_b, float(burst_prob), z1, u, z2, self.var_to_factors, self.factor_to_vars,
                  B, self.N, self.M, self.dv, self.dc, _hip.dtype_code(node), y, node, hop, ef_f2v, ef_v2f)
        return y, node, hop, ef_f2v, ef_v2f

    def received_features(self, y, snr_db, dtype=torch.float32):
        """Model inputs from given received words (the reference's ``Codes.__getitem__``, lib/data/ldpc_dataset.py:141-156, over a
        batch): y [B,96] and snr_db [B] (one value per word) or [B,96] (the stored per-bit ``snr_dbs`` rows; node row 1 is that row).
        Returns (node_feature [B,2,96,1], hop_feature [B,6,48,1], efeature_f2v [B,7,96,3], efeature_v2f [B,7,48,6]) in ``dtype``:
        on the ``y`` that ``channel_features`` returns, exactly that call's four feature tensors."""
        B = check_received_args(y, snr_db, dtype, self.N)
        dev = self.device
        y = y.to(dev, torch.float32).contiguous()
        snr_db = snr_db.to(dev, torch.float32).contiguous()
        snr_sb, snr_sn = (1, 0) if snr_db.dim() == 1 else (self.N, 1)
        node, hop, ef_f2v, ef_v2f = self._features(B, dtype)
        _hip.call('fgnn_ldpc_received_features', y, snr_db, snr_sb, snr_sn, self.var_to_factors, self.factor_to_vars, B, self.N, self.M,
                  self.dv, self.dc, _hip.dtype_code(node), node, hop, ef_f2v, ef_v2f)
        return node, hop, ef_f2v, ef_v2f

    def make_test_set(self, num, seed=0, snr_db=(0, 1, 2, 3, 4), sigma_b=(0, 1, 2, 3, 4, 5), burst_prob=0.05, baseline=True):
        """A test set as the reference's generator writes it (data_generate/ldpc.py:45-89): ``num`` items per class of (SNR, burst
        sigma_b), sigma_b outer, SNR inner.  Returns CPU tensors: ``noizy_sg`` f32 [n,96] (received words), ``gts`` int64 [n,96]
        (the transmitted codewords), ``snr_dbs`` f32 [n,96] (constant rows), ``sigma_b`` f32 [n]; with ``baseline`` also
        ``sp_error``, float64 [n_snr, n_sigma]: the generator's ``error`` table, the sum-product decoder's mean message-bit error per
        class (``decode(bit_prior(y, snr), loops=100)``, lib/data/ldpc.py:18-24).

        Reproducible from the arguments: the messages come from ``torch.Generator(device).manual_seed(seed)`` (one draw of [n,48]);
        the channel's draws from the feature kernel's own generator (``channel_features(kernel_rng=(seed, 2**62 + k))`` for the k-th
        chunk of at most 4096 items).  Why 2**62: small offsets are a training loop's step numbers (``sample(kernel_rng=True,
        step=...)``), so test words never reuse a training batch's noise; and bit 63 of the offset selects the kernel's second (z2)
        stream, so offsets stay below 2**63."""
        snr_db, sigma_b = check_grids(snr_db, sigma_b)
        num = int(num)
        if num < 1:
            raise ValueError('num must be >= 1, got %d' % num)
        dev = self.device
        nc = len(snr_db) * len(sigma_b)
        n = num * nc
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        s = torch.randint(0, 2, (n, self.K), device=dev, generator=gen, dtype=torch.uint8)
        cw = self.encode(s)
        snr_cls = torch.tensor([float(v) for _ in sigma_b for v in snr_db], dtype=torch.float32)      # sigma_b outer, SNR inner
        sb_cls = torch.tensor([float(v) for v in sigma_b for _ in snr_db], dtype=torch.float32)
        snr = snr_cls.repeat_interleave(num).to(dev)
        sb = sb_cls.repeat_interleave(num).to(dev)
        y = torch.empty((n, self.K + self.P), device=dev, dtype=torch.float32)
        chunk = 4096
        for k in range(0, (n + chunk - 1) // chunk):
            i, j = k * chunk, min(n, (k + 1) * chunk)
            y[i:j] = self.channel_features(cw[i:j], snr[i:j], sb[i:j], burst_prob, kernel_rng=(seed, 2 ** 62 + k))[0]
        out = {'noizy_sg': y.cpu(), 'gts': cw.long().cpu(), 'snr_dbs': snr[:, None].expand(-1, self.N).contiguous().cpu(),
               'sigma_b': sb.cpu()}
        if baseline:
            from .ldpc_eval import LdpcErrorCounts      # (here: ldpc_eval imports this module)
            acc, mackay = LdpcErrorCounts(dev, snr_db, sigma_b), parse_decoder('mackay')
            for i in range(0, n, chunk):
                j = min(n, i + chunk)
                x = mackay.run(self, y[i:j], snr[i:j])[0]
                acc.add_bits(x, cw[i:j], snr[i:j], sb[i:j], nbits=self.K)
            out['sp_error'] = torch.from_numpy(acc.result()['err_class'])
        return out

    def write_test_set(self, path, num, seed=0, snr_db=(0, 1, 2, 3, 4), sigma_b=(0, 1, 2, 3, 4, 5), burst_prob=0.05, baseline=True):
        """``make_test_set`` saved with ``torch.save`` as the reference's generator saves it: the four keys ``noizy_sg``, ``gts``,
        ``snr_dbs``, ``sigma_b`` only, so the unchanged ``lib.data.Codes(path)`` (and ``train_ldpc.py --test_path``) reads it.
        Returns the sum-product table (``sp_error``) when ``baseline``, else None."""
        d = self.make_test_set(num, seed, snr_db, sigma_b, burst_prob, baseline)
        torch.save({k: d[k] for k in ('noizy_sg', 'gts', 'snr_dbs', 'sigma_b')}, path)
        return d.get('sp_error')

    def sample(self, B, seed=0, dtype=torch.float32, snr_db=None, burst_prob=0.05, kernel_rng=False, step=0):
        """A batch of B training items (ldpc_dataset.py:222-236): random messages, encoded, sent through the
        channel at a per-item SNR drawn from ``snr_db_choices`` (or the fixed ``snr_db``) and burst level from
        ``sigma_b_choices``.  Returns (node_feature, hop_feature, nn_idx_f2v [B,96,3], nn_idx_v2f [B,48,6],
        efeature_f2v, efeature_v2f, label [B,96] int64 = the transmitted codeword, sigma_b [B])."""
        gen = torch.Generator(device=self.device).manual_seed(seed)
        s = torch.randint(0, 2, (B, self.K), device=self.device, generator=gen, dtype=torch.uint8)
        cw = self.encode(s)
        pick = lambda choices: torch.tensor(choices, device=self.device, dtype=torch.float32)[
            torch.randint(0, len(choices), (B,), device=self.device, generator=gen)]
        snr = pick(self.snr_db_choices) if snr_db is None else torch.full((B,), float(snr_db), device=self.device)
        sigma_b = pick(self.sigma_b_choices)
        # kernel_rng: the channel's draws are made inside the feature kernel from (seed, step) instead of three noise tensors
        _, node, hop, ef_f2v, ef_v2f = self.channel_features(cw, snr, sigma_b, burst_prob, generator=gen, dtype=dtype,
                                                             kernel_rng=(seed, step) if kernel_rng else None)
        return (node, hop, self.nn_idx_f2v.unsqueeze(0).expand(B, -1, -1), self.nn_idx_v2f.unsqueeze(0).expand(B, -1, -1),
                ef_f2v, ef_v2f, cw.long(), sigma_b)


    def sample_rng(self, B, seed=0, step=0, dtype=torch.float32, snr_db=None, burst_prob=0.05, out=None):
        """A NEW batch of B training items per ``step`` in ONE launch (fgnn_ldpc_sample_rng, include/fgnn_hip_ldpc_train.h;
        ``ContinousCodesSP.__getitem__``, ldpc_dataset.py:222-236, over a batch): messages, SNR classes (``snr_db_choices``, or the one
        value ``snr_db``) and burst classes (``sigma_b_choices``) come from one Philox block per codeword keyed by ``seed`` at counter
        (b, ``step``), the channel's draws from the feature kernel's generator at the same (seed, step).  No torch generator.

        Returns an ``LdpcBatch``: (node_feature, hop_feature, nn_idx_f2v, nn_idx_v2f, efeature_f2v, efeature_v2f, label [B,48] f32 =
        the message bits, sigma_b [B]) as ``sample`` orders them (the index tables are its expanded stride-0 views), then snr_db [B],
        cw [B,96] uint8 and y [B,96] f32.  ``out``: a previous result for the same (B, dtype); every tensor is written in place and
        ``out`` itself is returned, so a captured step reads the same buffers each step with no copies."""
        snr_choices = self.snr_db_choices if snr_db is None else (snr_db,)
        check_sample_rng_args(B, seed, step, dtype, snr_choices, self.sigma_b_choices, out)
        B, dev, N = int(B), self.device, self.K + self.P
        if out is None:
            new = lambda *shape, dt=dtype: torch.empty(shape, device=dev, dtype=dt)
            out = LdpcBatch(new(B, 2, N, 1), new(B, self.dc, self.M, 1), self.nn_idx_f2v.unsqueeze(0).expand(B, -1, -1),
                            self.nn_idx_v2f.unsqueeze(0).expand(B, -1, -1), new(B, self.dc + 1, N, self.dv),
                            new(B, self.dc + 1, self.M, self.dc),
                            new(B, self.K, dt=torch.float32), new(B, dt=torch.float32), new(B, dt=torch.float32),
                            new(B, N, dt=torch.uint8), new(B, N, dt=torch.float32))
        farr = lambda c: (ctypes.c_float * len(c))(*[float(v) for v in c])
        name, sizes = (('fgnn_ldpc_sample_rng', (B, self.K, self.P)) if self.one_word else
                       ('fgnn_ldpc_sample_rng_words', (B, self.K, self.P, self.W)))
        _hip.call(name, int(seed), int(step), farr(snr_choices), len(snr_choices), farr(self.sigma_b_choices),
                  len(self.sigma_b_choices), float(burst_prob), self.gmask, self.var_to_factors, self.factor_to_vars, *sizes,
                  self.M, self.dv, self.dc, _hip.F32 if dtype == torch.float32 else _hip.BF16, out.node_feature, out.hop_feature,
                  out.efeature_f2v, out.efeature_v2f, out.snr_db, out.sigma_b, out.cw, out.label, out.y)
        return out


def check_received_args(y, snr_db, dtype, n_var=96):
    """Shapes of ``LdpcDataPath.received_features`` for a code of ``n_var`` variables (before anything reaches the device): returns B."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('dtype must be float32 or bfloat16')
    if y.dim() != 2 or y.shape[1] != n_var:
        raise ValueError('received words must be [B, %d], got %s' % (n_var, tuple(y.shape),))
    B = y.shape[0]
    if tuple(snr_db.shape) not in ((B,), (B, n_var)):
        raise ValueError('snr_db must be [B] or [B, %d] with B = %d, got %s' % (n_var, B, tuple(snr_db.shape)))
    return B


def check_grids(snr_grid, sigma_grid):
    """The class grids of the test loop: SNR values (dB, float) and integer burst levels, at least one of each and at most 256
    classes (fgnn_ldpc_error_counts).  Returns them as tuples of float and int."""
    snr_grid, sigma_grid = tuple(snr_grid), tuple(sigma_grid)
    if not snr_grid or not sigma_grid:
        raise ValueError('empty class grid')
    if len(snr_grid) * len(sigma_grid) > 256:
        raise ValueError('at most 256 classes, got %d x %d' % (len(snr_grid), len(sigma_grid)))
    if any(not np.isfinite(float(v)) for v in snr_grid):
        raise ValueError('SNR grid values must be finite')
    if any(not np.isfinite(float(v)) or float(v) != int(v) or abs(int(v)) >= 2 ** 31 for v in sigma_grid):
        raise ValueError('sigma_b grid values must be 32-bit integers, got %s' % (sigma_grid,))
    return tuple(float(v) for v in snr_grid), tuple(int(v) for v in sigma_grid)
