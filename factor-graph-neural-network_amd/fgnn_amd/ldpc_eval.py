"""Decoding quality of LDPC decoders on the GPU: the reference's test loop and its test-set generator.

The reference judges a trained decoder with ``train_ldpc.py:test()`` (/root/reference/train_ldpc.py:262-327): it reads a stored test
set through ``lib.data.Codes``, runs the model in batches of 100 and prints the overall bit error rate of the 48 message bits and a
5 x 6 table of bit error rates per class of (SNR in {0..4} dB, burst level sigma_b in {0..5}).  The test set comes from
``data_generate/ldpc.py``, which prints the same table for the classical sum-product decoder beside it.

Here the whole loop stays on the device: ``LdpcDataPath.received_features`` builds the model inputs from the stored received words,
``LdpcErrorCounts`` accumulates the counts with one launch per batch (csrc/ldpc_eval.hip) and reads them back once, and
``LdpcDataPath.make_test_set`` / ``write_test_set`` generate test sets.  The classical decoders evaluated beside a model are
``ldpc_decoders.parse_decoder``'s ``Decoder`` values.  ``python -m fgnn_amd.ldpc_eval`` is the command line.
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

from . import _hip
from .datapath import LdpcDataPath, check_grids
from .ldpc import LDPCModel
from .ldpc_code import LdpcCode
from .ldpc_decoders import parse_decoder
from .ldpc_train import build_model

SNR_GRID = (0, 1, 2, 3, 4)              # train_ldpc.py:298 (SNR) and the acc_cnt rows
SIGMA_GRID = (0, 1, 2, 3, 4, 5)         # train_ldpc.py:320 (range(6)) and the acc_cnt columns
COLUMNS = ('bits', 'bit_errors', 'words', 'word_errors')


def check_count_args(dec, label, snr_db, sigma_b, nbits):
    """Shapes and dtypes of one ``LdpcErrorCounts`` batch (before anything reaches the device): decisions [B, >= nbits], labels
    [B, >= nbits] int64 / uint8 / bool, snr_db [B] or [B, k] (column 0 classifies, as the reference's node_feature[:, 1, 0, 0]),
    sigma_b [B].  Returns B."""
    nbits = int(nbits)
    if not 1 <= nbits <= 1024:
        raise ValueError('nbits must be in 1..1024, got %d' % nbits)
    if dec.dim() != 2 or dec.shape[1] < nbits:
        raise ValueError('decisions must be [B, >= %d], got %s' % (nbits, tuple(dec.shape)))
    B = dec.shape[0]
    if label.dim() != 2 or label.shape[0] != B or label.shape[1] < nbits:
        raise ValueError('labels must be [%d, >= %d], got %s' % (B, nbits, tuple(label.shape)))
    if label.dtype not in (torch.int64, torch.uint8, torch.bool):
        raise ValueError('labels must be int64, uint8 or bool, got %s' % label.dtype)
    if not (snr_db.dim() == 1 and snr_db.shape[0] == B) and not (snr_db.dim() == 2 and snr_db.shape[0] == B and snr_db.shape[1] >= 1):
        raise ValueError('snr_db must be [%d] or [%d, k], got %s' % (B, B, tuple(snr_db.shape)))
    if tuple(sigma_b.shape) != (B,):
        raise ValueError('sigma_b must be [%d], got %s' % (B, tuple(sigma_b.shape)))
    return B


class LdpcErrorCounts:
    """Bit and word error counts of LDPC decisions per class of (SNR, sigma_b), accumulated on the device.

    ``add_logits`` / ``add_bits`` only enqueue one launch of ``fgnn_ldpc_error_counts``; ``result()`` synchronises once.  The
    classes are those of train_ldpc.py:316-324: the first SNR grid value within 1e-3 of the word's SNR (of bit 0) and the sigma_b
    grid value equal to ``int(sigma_b)`` (truncated, as ``sigma_b.long()``); a word outside every class counts only overall."""

    def __init__(self, device, snr_grid=SNR_GRID, sigma_grid=SIGMA_GRID):
        self.snr_grid, self.sigma_grid = check_grids(snr_grid, sigma_grid)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('LdpcErrorCounts runs on a ROCm device (no CPU fallback)')
        self._snr = torch.tensor(self.snr_grid, dtype=torch.float32, device=self.device)
        self._sigma = torch.tensor(self.sigma_grid, dtype=torch.int32, device=self.device)
        self.counts = torch.zeros((len(self.snr_grid) * len(self.sigma_grid) + 1, 4), dtype=torch.int64, device=self.device)

    def reset(self):
        self.counts.zero_()

    def add_logits(self, logits, label, snr_db, sigma_b, nbits=48):
        """A model's logits [B, >= nbits] f32 / bf16: bit = logit >= 0 (the reference's test, train_ldpc.py:302)."""
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('logits must be float32 or bfloat16, got %s' % logits.dtype)
        self._add(logits, _hip.DEC_F32 if logits.dtype == torch.float32 else _hip.DEC_BF16, label, snr_db, sigma_b, nbits)

    def add_bits(self, x, label, snr_db, sigma_b, nbits=48):
        """Hard decisions [B, >= nbits] uint8 / bool (bit = x != 0), such as ``LdpcDataPath.decode``'s."""
        if x.dtype not in (torch.uint8, torch.bool):
            raise ValueError('hard decisions must be uint8 or bool, got %s' % x.dtype)
        self._add(x.view(torch.uint8) if x.dtype == torch.bool else x, _hip.DEC_U8, label, snr_db, sigma_b, nbits)

    def _add(self, dec, kind, label, snr_db, sigma_b, nbits):
        B = check_count_args(dec, label, snr_db, sigma_b, nbits)
        if B == 0:
            return
        dev = self.device
        dec = dec.to(dev)
        if dec.stride(1) != 1:
            dec = dec.contiguous()
        label = label.to(dev)
        if label.dtype == torch.bool:
            label = label.view(torch.uint8)
        if label.stride(1) != 1:
            label = label.contiguous()
        snr_db = snr_db.to(dev, torch.float32)
        snr0 = snr_db if snr_db.dim() == 1 else snr_db[:, 0]
        sigma_b = sigma_b.to(dev, torch.float32).contiguous()
        _hip.call('fgnn_ldpc_error_counts', dec, kind, dec.stride(0), label,
                  _hip.LABEL_I64 if label.dtype == torch.int64 else _hip.LABEL_U8, label.stride(0), snr0, snr0.stride(0), sigma_b, B,
                  int(nbits), self._snr, len(self.snr_grid), self._sigma, len(self.sigma_grid), self.counts)

    def result(self):
        """One read-back.  ``ber``: 1 - right / compared over every word (train_ldpc.py:326); ``err_class`` [n_snr, n_sigma]:
        1 - acc_cnt / acc_tot (train_ldpc.py:327; NaN for an empty class); ``fer`` / ``fer_class``: the same for whole words;
        ``counts`` [n_snr * n_sigma + 1, 4] int64 (columns bits, bit errors, words, word errors; rows SNR-major, the last overall)."""
        c = self.counts.cpu().numpy()
        ns, nb = len(self.snr_grid), len(self.sigma_grid)
        cls = c[:-1].reshape(ns, nb, 4).astype(np.float64)
        tot = c[-1]
        with np.errstate(divide='ignore', invalid='ignore'):
            err_class = 1 - np.divide(cls[..., 0] - cls[..., 1], cls[..., 0])
            fer_class = np.divide(cls[..., 3], cls[..., 2])
        return {'ber': 1 - int(tot[0] - tot[1]) / int(tot[0]) if tot[0] else float('nan'),
                'err_class': err_class,
                'fer': int(tot[3]) / int(tot[2]) if tot[2] else float('nan'),
                'fer_class': fer_class,
                'counts': c}


class MlCertificates:
    """What only the plain LP decoder (``Decoder.certifies``) can count, accumulated on the device: ``ml_certified``, the words whose
    flags carry the ML certificate (bit 1 of ``LdpcDecoders.decode_lp``'s), and ``certified_word_errors``, those among them that differ
    from the sent word: each is a word on which the maximum-likelihood decoder errs too, so their number is a lower bound on its
    word errors."""

    def __init__(self, device):
        self.counts = torch.zeros(2, dtype=torch.int64, device=device)

    def add(self, x, flags, sent):
        """x [B, N] hard decisions, flags [B], sent [B, N] the transmitted words."""
        cert = (flags & 2) != 0
        wrong = (x != sent.to(x.device)[:, :x.shape[1]].to(x.dtype)).any(1)
        self.counts += torch.stack((cert.sum(), (cert & wrong).sum()))

    def result(self):
        ml_certified, certified_word_errors = self.counts.tolist()
        return {'ml_certified': ml_certified, 'certified_word_errors': certified_word_errors}


def run_counted(decoder, path, y, snr0, sent, certs):
    """``decoder.run(path, y, snr0)``; a decoder that certifies also adds its flags against ``sent`` to ``certs`` (an
    ``MlCertificates``)."""
    if not decoder.certifies:
        return decoder.run(path, y, snr0)
    x, viol, iters, flags = decoder.run_flags(path, y, snr0)
    certs.add(x, flags, sent)
    return x, viol, iters


def load_test_set(test_set, device, n_var=96):
    """A test set (the dict of ``make_test_set`` / the reference's generator, or a path to its ``torch.save`` file) on ``device``:
    (noizy_sg [n,96] f32, gts [n,96], snr_dbs [n,96] or [n] f32, sigma_b [n] f32); 96 reads ``n_var`` for another code."""
    if isinstance(test_set, (str, os.PathLike)):
        test_set = torch.load(test_set, map_location='cpu')
    y, gts, snr, sb = (test_set[k] for k in ('noizy_sg', 'gts', 'snr_dbs', 'sigma_b'))
    n, N = y.shape[0], int(n_var)
    if tuple(y.shape) != (n, N) or tuple(gts.shape) != (n, N) or tuple(snr.shape) not in ((n, N), (n,)) or tuple(sb.shape) != (n,):
        raise ValueError('test set shapes: noizy_sg %s, gts %s, snr_dbs %s, sigma_b %s (want [n,%d], [n,%d], [n,%d] or [n], [n])'
                         % (tuple(y.shape), tuple(gts.shape), tuple(snr.shape), tuple(sb.shape), N, N, N))
    if gts.dtype not in (torch.int64, torch.uint8):
        gts = gts.long()
    return (y.to(device, torch.float32), gts.to(device), snr.to(device, torch.float32), sb.to(device, torch.float32))


def load_model(model_path, code=None, aggregator='max', device='cpu'):
    """The model of a checkpoint (``ldpc_train``'s or the reference script's) for ``code`` (None: the built-in 96.3.963).  A checkpoint
    trained for another code — its 'code' entry, or the lack of one, says which — is refused with a ValueError."""
    code = LdpcCode.builtin() if code is None else code
    ckpt = torch.load(model_path, map_location='cpu', weights_only=True)
    code.check_checkpoint(ckpt, model_path)
    model = build_model(aggregator, code)
    model.load_state_dict(ckpt['model_state_dict'], strict=True)
    return model.to(device)


def evaluate(model, test_set, batch_size=4096, dtype=torch.float32, baseline=False, snr_grid=SNR_GRID, sigma_grid=SIGMA_GRID, code=None):
    """``train_ldpc.py:test()`` for an ``fgnn_amd.LDPCModel`` on a test set (dict or path): the model in eval mode under no_grad
    (bf16: bf16 features under bf16 autocast), ``batch_size`` words per batch, nothing read back to the host until the end.  Returns
    ``LdpcErrorCounts.result()`` of the model's logits; with ``baseline`` also, under 'baseline', that of the sum-product decoder
    (``decode(bit_prior(y, snr), loops=100)``, lib/data/ldpc.py:18-24) on the same received words.  The model's training flag is
    restored afterwards.  ``baseline`` may also be a decoder spec (``parse_decoder``: 'mackay', 'min-sum:layered', ...): that decoder's
    result under 'baseline'; or a list of specs: one result each under ``res['baselines'][spec]``.  ``code``: the ``LdpcCode`` the model was built for (None: the built-in 96.3.963); the errors are counted
    over its K message bits and the baseline runs on its ``nlist``.  ``model`` may also be a checkpoint's path (``load_model``).  The
    result of a plain LP decoder ('admm-lp' with penalty 0) also carries ``ml_certified`` and ``certified_word_errors``
    (``MlCertificates``)."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('dtype must be float32 or bfloat16')
    if baseline is True:
        baseline = 'mackay'         # the sum-product table is that spec's
    specs = () if baseline is None or baseline is False else (baseline,) if isinstance(baseline, str) else tuple(baseline)
    parsed = [parse_decoder(spec) for spec in specs]
    if len(set(specs)) != len(specs):
        raise ValueError('baseline lists a decoder twice: %s' % (specs,))
    code = LdpcCode.builtin() if code is None else code
    if isinstance(model, (str, os.PathLike)):
        model = load_model(model, code, device='cuda')
    if (getattr(model, 'n_var', code.n_var), getattr(model, 'n_msg', code.K)) != (code.n_var, code.K):
        raise ValueError('the model decodes %d of %d variables, %r has K = %d of N = %d: pass the code the model was built for'
                         % (model.n_msg, model.n_var, code, code.K, code.n_var))
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError('batch_size must be >= 1')
    dev = next(model.parameters()).device
    counts = LdpcErrorCounts(dev, snr_grid, sigma_grid)
    decoders = [(spec, decoder, LdpcErrorCounts(dev, snr_grid, sigma_grid), MlCertificates(dev)) for spec, decoder in zip(specs, parsed)]
    result = lambda decoder, acc, certs: dict(acc.result(), **(certs.result() if decoder.certifies else {}))
    path = LdpcDataPath(dev, code)
    y, gts, snr, sb = load_test_set(test_set, dev, code.n_var)
    n = y.shape[0]
    was = model.training
    model.eval()
    try:
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            for i in range(0, n, batch_size):
                j = min(n, i + batch_size)
                B = j - i
                node, hop, ef_f2v, ef_v2f = path.received_features(y[i:j], snr[i:j], dtype)
                logits, _ = model(node, hop, path.nn_idx_f2v.unsqueeze(0).expand(B, -1, -1),
                                  path.nn_idx_v2f.unsqueeze(0).expand(B, -1, -1), ef_f2v, ef_v2f)
                counts.add_logits(logits, gts[i:j], snr[i:j], sb[i:j], nbits=code.K)
                snr0 = snr[i:j] if snr.dim() == 1 else snr[i:j, 0]
                for _, decoder, acc, certs in decoders:
                    acc.add_bits(run_counted(decoder, path, y[i:j], snr0, gts[i:j], certs)[0], gts[i:j], snr[i:j], sb[i:j], nbits=code.K)
    finally:
        model.train(was)
    res = counts.result()
    if isinstance(baseline, str):
        res['baseline'] = result(*decoders[0][1:])
    elif decoders:
        res['baselines'] = {spec: result(decoder, acc, certs) for spec, decoder, acc, certs in decoders}
    return res


def ber_curve(code, decoder, snr_db, sigma_b=0, batch=4096, min_word_errors=100, max_words=10 ** 6, seed=0, device='cuda:0'):
    """A BER / WER-versus-SNR curve of one classical decoder (a ``parse_decoder`` spec) on ``code`` (an ``LdpcCode``; None: the
    built-in one).  Per SNR value, batches of ``batch`` words are drawn with ``LdpcDataPath.sample_rng(batch, seed, step, snr_db=that
    value)`` on a data path whose ``sigma_b_choices`` is the one level ``sigma_b``, decoded from the drawn ``y`` and counted against
    the drawn ``cw`` over the K message bits (``LdpcErrorCounts``), until the first batch boundary at which the word errors reach
    ``min_word_errors`` or the words reach ``max_words``.  The counts are read back once per batch (the stopping rule needs them).

    Reproducible from the arguments: the j-th batch (j = 0, 1, ...) of the i-th SNR value (in the order given) is
    ``sample_rng(batch, seed=seed, step=i * 2**32 + j)``, so no two batches of a curve share their draws (at most 2**32 batches per
    point).  Returns a list of dicts, one per SNR value: snr_db, words, bit_errors, word_errors, ber, wer, mean_iters, and for a plain LP
    decoder ('admm-lp' with penalty 0) ml_certified and certified_word_errors (``MlCertificates``)."""
    code = LdpcCode.builtin() if code is None else code
    decoder = parse_decoder(decoder)
    snr_db = [float(v) for v in ([snr_db] if np.isscalar(snr_db) else snr_db)]
    (_, ), (sigma_b,) = check_grids((0.0,), (sigma_b,))
    batch, min_word_errors, max_words = int(batch), int(min_word_errors), int(max_words)
    if not snr_db or any(not np.isfinite(v) for v in snr_db):
        raise ValueError('snr_db: at least one finite value, got %s' % (snr_db,))
    if batch < 1 or min_word_errors < 1 or max_words < 1:
        raise ValueError('batch, min_word_errors and max_words must be >= 1')
    path = LdpcDataPath(device, code)
    path.sigma_b_choices = (sigma_b,)
    out = []
    for i, snr in enumerate(snr_db):
        acc = LdpcErrorCounts(path.device, (snr,), (sigma_b,))
        it_sum = torch.zeros((), dtype=torch.int64, device=path.device)
        certs = MlCertificates(path.device)
        drawn = None
        for j in range(2 ** 32):
            drawn = path.sample_rng(batch, seed=seed, step=i * 2 ** 32 + j, snr_db=snr, out=drawn)
            x, _, iters = run_counted(decoder, path, drawn.y, drawn.snr_db, drawn.cw, certs)
            acc.add_bits(x, drawn.cw, drawn.snr_db, drawn.sigma_b, nbits=code.K)
            it_sum += iters.sum()
            tot = acc.counts[-1].tolist()
            if tot[3] >= min_word_errors or tot[2] >= max_words:
                break
        bits, bit_errors, words, word_errors = tot
        out.append({'snr_db': snr, 'words': words, 'bit_errors': bit_errors, 'word_errors': word_errors, 'ber': bit_errors / bits,
                    'wer': word_errors / words, 'mean_iters': int(it_sum) / words, **(certs.result() if decoder.certifies else {})})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m fgnn_amd.ldpc_eval',
                                 description='Evaluate an LDPC decoder on a stored test set (train_ldpc.py --test_path) or write a '
                                             'test set (data_generate/ldpc.py).')
    ap.add_argument('--test_path', help='test set to evaluate on (torch.save dict: noizy_sg, gts, snr_dbs, sigma_b)')
    ap.add_argument('--model_path', help="checkpoint with 'model_state_dict' (train_ldpc.py's format)")
    ap.add_argument('--batch_size', type=int, default=4096)
    ap.add_argument('--aggregator', default='max')
    ap.add_argument('--dtype', choices=('f32', 'bf16'), default='f32')
    ap.add_argument('--baseline', action='store_true', help='also print the sum-product decoder\'s table')
    ap.add_argument('--decoder', action='append', default=[], metavar='SPEC',
                    help='also print the table of a classical decoder; may be repeated.  mackay, or min-sum | offset-min-sum | '
                         'sum-product [:flooding | :layered] [:iters=N] [:alpha=A] [:beta=B] [:osd=W [:span=L]] (osd: ordered-'
                         'statistics reprocessing of order W), or learned-min-sum:CHECKPOINT (python -m fgnn_amd.ldpc_nms_train; runs the '
                         'schedule the checkpoint was trained with, flooding or layered), or admm-lp [:iters=N] [:mu=M] [:penalty=A] '
                         '[:relax=R] [:eps=E] [:osd=W [:span=L]] (the ADMM linear-programming decoder; with penalty 0 the words it '
                         'certifies as maximum-likelihood are counted too)')
    ap.add_argument('--curve', action='store_true', help='print a BER / WER curve of the one --decoder over --snr (no model)')
    ap.add_argument('--snr', default='0,1,2,3,4', help='--curve: SNR values in dB, comma-separated')
    ap.add_argument('--sigma_b', type=int, default=0, help='--curve: the burst level')
    ap.add_argument('--min_word_errors', type=int, default=100, help='--curve: stop a point at this many word errors ...')
    ap.add_argument('--max_words', type=int, default=10 ** 6, help='--curve: ... or at this many words')
    ap.add_argument('--make_test_set', metavar='P', help='write a test set to P and print the sum-product table')
    ap.add_argument('--num', type=int, default=1000, help='items per class (--make_test_set)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--burst_prob', type=float, default=0.05)
    ap.add_argument('--code', default='builtin', help='builtin (96.3.963), the path of an alist file, or gallager:N,dv,dc,seed')
    args = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    code = LdpcCode.from_spec(args.code)
    if args.make_test_set:
        sp = LdpcDataPath(dev, code).write_test_set(args.make_test_set, args.num, seed=args.seed, burst_prob=args.burst_prob)
        print(sp)
        return 0
    if args.curve:
        if len(args.decoder) != 1:
            ap.error('--curve takes exactly one --decoder')
        rows = ber_curve(code, args.decoder[0], [float(v) for v in args.snr.split(',')], args.sigma_b, args.batch_size,
                         args.min_word_errors, args.max_words, args.seed, dev)
        certifies = 'ml_certified' in rows[0]       # (the plain LP decoder: two more columns)
        print('%8s %10s %12s %12s %12s %12s %10s' % ('snr_db', 'words', 'bit_errors', 'word_errors', 'ber', 'wer', 'mean_iters')
              + (' %12s %10s' % ('ml_certified', 'cert_wrong') if certifies else ''))
        for r in rows:
            print('%8.3f %10d %12d %12d %12.4e %12.4e %10.3f' % (r['snr_db'], r['words'], r['bit_errors'], r['word_errors'], r['ber'],
                                                               r['wer'], r['mean_iters'])
                  + (' %12d %10d' % (r['ml_certified'], r['certified_word_errors']) if certifies else ''))
        return 0
    if not args.test_path or not args.model_path:
        ap.error('give --test_path and --model_path, or --make_test_set, or --curve')
    if code.is_default:
        with contextlib.redirect_stdout(sys.stderr):           # (the model's construction talks; stdout carries the result only)
            model = LDPCModel(2, 6, 4, aggregator=args.aggregator)
        ckpt = torch.load(args.model_path, map_location=dev)
        code.check_checkpoint(ckpt, args.model_path)
        model.load_state_dict(ckpt['model_state_dict'])
        model.to(dev)
    else:
        model = load_model(args.model_path, code, args.aggregator, dev)
    # one pass over the test set: with --decoder the sum-product table of --baseline is the 'mackay' spec's (the same decoder call)
    specs = (['mackay'] if args.baseline and 'mackay' not in args.decoder else []) + args.decoder
    res = evaluate(model, args.test_path, args.batch_size, torch.bfloat16 if args.dtype == 'bf16' else torch.float32,
                   baseline=specs if args.decoder else args.baseline, code=code)
    print(res['ber'])
    print(torch.FloatTensor(res['err_class']))
    if args.baseline:
        print(torch.FloatTensor((res['baselines']['mackay'] if args.decoder else res['baseline'])['err_class']))
    for spec in args.decoder:
        print(spec)
        print(torch.FloatTensor(res['baselines'][spec]['err_class']))
        if 'ml_certified' in res['baselines'][spec]:
            r = res['baselines'][spec]
            print('ml_certified %d of %d words, certified_word_errors %d (a lower bound on the ML decoder\'s word errors)'
                  % (r['ml_certified'], int(r['counts'][-1][2]), r['certified_word_errors']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
