"""The classical LDPC decoders: everything on the host that drives a decoder kernel.

``LdpcDecoders``, the base class of ``datapath.LdpcDataPath``, carries the probability-domain sum-product decoder (``decode``,
csrc/ldpc_decode.hip), the LLR-domain decoders (``decode_llr``, csrc/ldpc_llr.hip), the ADMM linear-programming decoder (``decode_lp``,
csrc/ldpc_lp.hip) and ordered-statistics reprocessing (``decode_osd``, csrc/ldpc_osd.hip) with their argument checks, mirrored limits
and the one set of device tables all four read.  ``parse_decoder``
turns a spec into a ``Decoder``, whose ``run`` decodes received words through a path.  ``ldpc_nms`` (the learned decoder) shares the
batch check and the output buffers.
"""
import collections
import typing

import numpy as np
import torch

from . import _hip

LLR_ALGORITHMS = {'min-sum': 0, 'offset-min-sum': 1, 'sum-product': 2}     # fgnn_ldpc_decode_llr's ``algorithm``
LLR_SCHEDULES = ('flooding', 'layered')
OSD_MAX_ORDER, OSD_MAX_PAIR_SPAN = 2, 256       # fgnn_ldpc_osd's limits (csrc/ldpc_osd.hip)
LP = 'admm-lp'                                  # the head of the ADMM-LP decoder's spec
LP_DEFAULTS = {'max_iter': 200, 'mu': 3.0, 'penalty': 0.0, 'relax': 1.9, 'eps': 1e-5}      # ``decode_lp``'s, and the spec's
LEARNED = 'learned-min-sum'                     # the head of the learned decoder's spec (``ldpc_nms.KIND``)

# a code's incidence tables on the device (``LdpcCode.incidence_tables``) and its sizes: what every decoder kernel is given
DecoderTables = collections.namedtuple('DecoderTables', 'col_ptr row_ptr row_edge row_var N M E')


def check_word_batch(what, t, n_var):
    """A batch of words as the decoders take it: ``t`` a floating-point [B, n_var] tensor of fewer than 2^31 words (``what`` names it
    in the messages).  Returns B."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != int(n_var):
        raise ValueError('%s must be a [B, %d] tensor, got %s' % (what, n_var, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    if not t.dtype.is_floating_point:
        raise ValueError('%s must be a floating-point tensor, got %s' % (what, t.dtype))
    if t.shape[0] >= 2 ** 31:
        raise ValueError('at most 2^31 - 1 words per call, got %d' % t.shape[0])
    return t.shape[0]


def check_decode_llr_args(llr, n_var, algorithm, schedule, max_iter, alpha, beta):
    """Arguments of ``LdpcDataPath.decode_llr`` (before anything reaches the device).  Returns (B, the algorithm's code)."""
    if algorithm not in LLR_ALGORITHMS:
        raise ValueError('algorithm must be one of %s, got %r' % (', '.join(LLR_ALGORITHMS), algorithm))
    if schedule not in LLR_SCHEDULES:
        raise ValueError('schedule must be one of %s, got %r' % (', '.join(LLR_SCHEDULES), schedule))
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= int(max_iter) < 2 ** 31:
        raise ValueError('max_iter must be an integer in [1, 2^31), got %r' % (max_iter,))
    for what, v in (('alpha', alpha), ('beta', beta)):
        if not (np.isfinite(float(v)) and 0 <= float(v) <= 3.0e38):
            raise ValueError('%s must be a finite float32 value >= 0, got %r' % (what, v))
    return check_word_batch('llr', llr, n_var), LLR_ALGORITHMS[algorithm]


def check_decode_lp_args(llr, n_var, min_degree, max_iter, mu, penalty, relax, eps, stop_on_codeword):
    """Arguments of ``LdpcDecoders.decode_lp`` (before anything reaches the device); ``min_degree``: the code's smallest positive
    variable degree, which 2 penalty / mu must stay below (the x-update divides by degree - 2 penalty / mu).  Returns (B,
    stop_on_codeword as 0 / 1, with None read as penalty > 0)."""
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= int(max_iter) < 2 ** 31:
        raise ValueError('max_iter must be an integer in [1, 2^31), got %r' % (max_iter,))
    if not (np.isfinite(float(mu)) and 0 < float(mu) <= 3.0e38):
        raise ValueError('mu must be a finite float32 value > 0, got %r' % (mu,))
    if not (np.isfinite(float(penalty)) and 0 <= float(penalty) <= 3.0e38):
        raise ValueError('penalty must be a finite float32 value >= 0, got %r' % (penalty,))
    if not (np.isfinite(float(eps)) and abs(float(eps)) <= 3.0e38):
        raise ValueError('eps must be a finite float32 value, got %r' % (eps,))
    if not 1 <= float(np.float32(relax)) < 2:
        raise ValueError('relax must be in [1, 2), got %r' % (relax,))
    if stop_on_codeword not in (None, False, True, 0, 1):
        raise ValueError('stop_on_codeword must be None, False or True, got %r' % (stop_on_codeword,))
    if not 2 * float(np.float32(penalty)) / float(np.float32(mu)) < min_degree:
        raise ValueError('2 penalty / mu = %g must be smaller than the smallest variable degree, %d' % (2 * float(penalty) / float(mu), min_degree))
    return check_word_batch('llr', llr, n_var), int(float(penalty) > 0 if stop_on_codeword is None else bool(stop_on_codeword))


def check_decode_osd_args(rel, metric, viol, n_var, order, span):
    """Arguments of ``LdpcDataPath.decode_osd`` (before anything reaches the device).  Returns (B, span with its default filled in:
    ``n_var`` for order 0 and 1, 64 for order 2)."""
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 0 <= int(order) <= OSD_MAX_ORDER:
        raise ValueError('order must be an integer in 0..%d, got %r' % (OSD_MAX_ORDER, order))
    if span is None:
        span = 64 if int(order) == 2 else int(n_var)
    if isinstance(span, bool) or not isinstance(span, (int, np.integer)) or not 1 <= int(span) < 2 ** 31:
        raise ValueError('span must be an integer in [1, 2^31), got %r' % (span,))
    if int(order) == 2 and int(span) > OSD_MAX_PAIR_SPAN:
        raise ValueError('span must be at most %d with order 2, got %d' % (OSD_MAX_PAIR_SPAN, span))
    B = check_word_batch('rel', rel, n_var)
    if metric is not None and check_word_batch('metric', metric, n_var) != B:
        raise ValueError('metric must hold rel\'s %d words, got %d' % (B, metric.shape[0]))
    if viol is not None:
        if not isinstance(viol, torch.Tensor) or tuple(viol.shape) != (B,) or viol.dtype != torch.int32:
            raise ValueError('viol must be a [%d] int32 tensor, got %s' % (B, '%s %s' % (tuple(viol.shape), viol.dtype) if isinstance(viol, torch.Tensor)
                                                                         else type(viol).__name__))
    return B, int(span)


def llr_batch(llr, device, n_var):
    """A checked [B, n_var] LLR batch as the decoder kernels read it: f32 on ``device``, unit column stride, rows that do not
    overlap (copied only where it is not)."""
    llr = llr.to(device, torch.float32)
    if llr.shape[0] and (llr.stride(1) != 1 or llr.stride(0) < n_var):
        llr = llr.contiguous()
    return llr


def decode_outputs(B, n_var, device, post_dtype=None):
    """A decoder's outputs, uninitialised: (x [B, n_var] uint8, posteriors [B, n_var] ``post_dtype`` or None, viol [B] int32,
    iters [B] int32)."""
    return (torch.empty((B, n_var), device=device, dtype=torch.uint8),
            None if post_dtype is None else torch.empty((B, n_var), device=device, dtype=post_dtype),
            torch.empty((B,), device=device, dtype=torch.int32), torch.empty((B,), device=device, dtype=torch.int32))


class LdpcDecoders:
    """The decoders of an ``LdpcDataPath`` (its base class; the path supplies ``device``, ``code`` and ``N``).  One set of device
    tables per path serves all four; each decoder's limits are checked on its first call, so a code may exceed one decoder only."""

    def __init__(self):
        self._tables = None             # DecoderTables, uploaded by the first decoder call
        self._layers = None             # (layer_ptr, layer_chk, n_layers) on the device, added by the first layered ``decode_llr``
        self._gated = set()             # the gates of ``_device_tables`` that have passed
        self._learned = {}              # checkpoint path -> its ``LearnedMinSum`` on the device (``learned``)

    def _device_tables(self, gate):
        """The device tables for the decoder ``gate`` names ('decode', 'llr', 'lp' or 'osd').  Its first call checks the code against
        that decoder's limits (``require_decoder`` / ``require_llr_decoder``, and for 'osd' and 'lp' the kernel's LDS footprint: the
        byte query refuses what does not fit); the first of any uploads ``code.incidence_tables()``."""
        if gate not in self._gated:
            (self.code.require_decoder if gate == 'decode' else self.code.require_llr_decoder)()
            if gate == 'osd' and int(_hip.invoke('fgnn_ldpc_osd_lds_bytes', self.code.n_var, self.code.n_chk)) < 0:
                raise ValueError(_hip.lib().fgnn_last_error().decode())
            if gate == 'lp' and int(_hip.invoke('fgnn_ldpc_decode_lp_lds_bytes', self.code.n_var, self.code.n_chk,
                                                int((np.asarray(self.code.nlist) >= 0).sum()))) < 0:
                raise ValueError(_hip.lib().fgnn_last_error().decode())
            if self._tables is None:
                tabs = self.code.incidence_tables()
                dev = lambda a: torch.from_numpy(a.copy()).to(self.device)      # (a copy: the code's arrays are read-only)
                self._tables = DecoderTables(*(dev(a) for a in tabs), self.code.n_var, self.code.n_chk, int(tabs[0][-1]))
            self._gated.add(gate)
        return self._tables

    def learned(self, checkpoint):
        """The ``LearnedMinSum`` of an ``ldpc_nms_train`` checkpoint on this path's device: loaded on the first call and kept (once per
        checkpoint path); one trained for another code than ``code`` is refused (``LdpcCode.check_checkpoint``)."""
        if checkpoint not in self._learned:
            from .ldpc_nms import load_checkpoint       # (here: ldpc_nms imports this module)
            self._learned[checkpoint] = load_checkpoint(checkpoint, self.code, self.device)
        return self._learned[checkpoint]

    def bit_prior(self, y, snr_db):
        """`y2b` (MNC_py.cpp:104-108): P(bit = 1 | y) = 1 / (1 + exp(-2 gcx y)), float64."""
        gcx = torch.pow(10.0, snr_db.to(self.device, torch.float64) / 20.0)[:, None]
        return 1.0 / (1.0 + torch.exp(-2.0 * gcx * y.to(self.device, torch.float64)))

    def decode(self, bias, loops=100, want_posteriors=False):
        """The reference's sum-product baseline `zb2x(bias, 48, 48, A2, 1, loops)` (lib/data/ldpc.py:18-24) for a
        batch: bias [B,96] float64 = P(bit = 1) (see ``bit_prior``).  Returns (x [B,96] uint8 hard decisions — the
        message is x[:, :48] —, violated checks [B] int32, iterations [B] int32[, q1 [B,96] float64])."""
        col_ptr, row_ptr, row_edge, row_var, N, M, E = self._device_tables('decode')
        if bias.dim() != 2 or bias.shape[1] != N:
            raise ValueError('bias must be [B, %d], got %s' % (N, tuple(bias.shape)))
        bias = bias.to(self.device, torch.float64).contiguous()
        B = bias.shape[0]
        x, q1, viol, iters = decode_outputs(B, N, self.device, torch.float64 if want_posteriors else None)
        _hip.call('fgnn_ldpc_decode', bias, col_ptr, row_ptr, row_edge, row_var, B, N, M, E, int(loops), x, q1, viol, iters)
        return (x, viol, iters, q1) if want_posteriors else (x, viol, iters)

    def bit_llr(self, y, snr_db):
        """The log-likelihood ratio of ``bit_prior``: log P(bit = 0 | y) / P(bit = 1 | y) = -2 gcx y with gcx = 10^(snr_db / 20), f32;
        y [B, N], snr_db [B]."""
        gcx = torch.pow(10.0, snr_db.to(self.device, torch.float32) / 20.0)[:, None]
        return -2.0 * gcx * y.to(self.device, torch.float32)

    def decode_llr(self, llr, algorithm='min-sum', schedule='flooding', max_iter=50, alpha=0.8125, beta=0.5, want_posteriors=False):
        """The LLR-domain decoders (fgnn_ldpc_decode_llr, include/fgnn_hip_ldpc_llr.h; no counterpart in the reference) for a batch:
        llr [B, N] = log P(bit = 0) / P(bit = 1) (see ``bit_llr``; f32, rows may be strided).  ``algorithm``: 'min-sum' (normalized
        by ``alpha``), 'offset-min-sum' (offset ``beta``) or 'sum-product'; ``schedule``: 'flooding', or 'layered' over
        ``code.layers()``.  Returns (x [B, N] uint8 hard decisions — the message is x[:, :K] —, violated checks [B] int32, iterations
        [B] int32[, post [B, N] f32: the final totals])."""
        B, alg = check_decode_llr_args(llr, self.N, algorithm, schedule, max_iter, alpha, beta)
        col_ptr, row_ptr, row_edge, row_var, N, M, E = self._device_tables('llr')
        layer_ptr, layer_chk, n_layers = None, None, 0
        if schedule == 'layered':
            if self._layers is None:
                lp, lc = self.code.layers()
                dev = lambda a: torch.from_numpy(np.array(a, np.int32)).to(self.device)       # (a copy: the code's arrays are read-only)
                self._layers = (dev(lp), dev(lc), len(lp) - 1)
            layer_ptr, layer_chk, n_layers = self._layers
        llr = llr_batch(llr, self.device, N)
        x, post, viol, iters = decode_outputs(B, N, self.device, torch.float32 if want_posteriors else None)
        _hip.call('fgnn_ldpc_decode_llr', llr, llr.stride(0) if B else N, col_ptr, row_ptr, row_edge, row_var, layer_ptr, layer_chk,
                  n_layers, B, N, M, E, alg, int(max_iter), float(alpha), float(beta), x, post, viol, iters)
        return (x, viol, iters, post) if want_posteriors else (x, viol, iters)

    def decode_lp(self, llr, max_iter=200, mu=3.0, penalty=0.0, relax=1.9, eps=1e-5, stop_on_codeword=None, want_soft=False):
        """The ADMM linear-programming decoder (fgnn_ldpc_decode_lp, include/fgnn_hip_ldpc_lp.h; no counterpart in the reference) for a
        batch: llr [B, N] as ``decode_llr`` takes it.  ``mu``: the ADMM step; ``penalty``: the weight of Liu & Draper's penalty term
        (0: the plain LP, whose integral optima are maximum-likelihood codewords); ``relax``: over-relaxation in [1, 2); a word stops
        when its primal residual and its change of z are both at most ``eps`` (never with eps < 0), or, with ``stop_on_codeword`` (None: penalty > 0), when
        its hard decisions satisfy every check, or after ``max_iter`` iterations.  2 penalty / mu must be smaller than the code's
        smallest variable degree.  Returns (x [B, N] uint8 hard decisions, violated checks [B] int32, iterations [B] int32, flags [B]
        int32: bit 0 = stopped by the residual rule, bit 1 = also integral to 1e-3, with penalty = 0 the ML certificate[, soft [B, N]
        f32: the final x in [0, 1])."""
        deg = (np.asarray(self.code.nlist) >= 0).sum(1)
        B, soc = check_decode_lp_args(llr, self.N, int(deg[deg > 0].min()), max_iter, mu, penalty, relax, eps, stop_on_codeword)
        col_ptr, row_ptr, row_edge, row_var, N, M, E = self._device_tables('lp')
        llr = llr_batch(llr, self.device, N)
        x, soft, viol, iters = decode_outputs(B, N, self.device, torch.float32 if want_soft else None)
        flags = torch.empty((B,), device=self.device, dtype=torch.int32)
        _hip.call('fgnn_ldpc_decode_lp', llr, llr.stride(0) if B else N, col_ptr, row_ptr, row_edge, row_var, B, N, M, E, int(max_iter),
                  float(mu), float(penalty), float(relax), float(eps), soc, x, soft, viol, iters, flags)
        return (x, viol, iters, flags, soft) if want_soft else (x, viol, iters, flags)

    def decode_osd(self, rel, metric=None, viol=None, order=1, span=None):
        """Ordered-statistics reprocessing (fgnn_ldpc_osd, include/fgnn_hip_ldpc_osd.h; no counterpart in the reference) for a batch:
        rel [B, N] orders the positions and gives the hard decisions (a decoder's posteriors: ``decode_llr(..., want_posteriors=True)``),
        ``metric`` [B, N] is what candidates are scored against (the channel LLRs, ``bit_llr``; None: rel), ``viol`` [B] int32 the
        decoder's violated checks: a word with none passes through (None: every word is reprocessed).  ``order`` 0, 1 or 2 over the
        ``span`` least reliable non-pivot positions (default: N for order 0 and 1, 64 for order 2; at most 256 with order 2).  Rows may
        be strided.  Returns (x [B, N] uint8 — every reprocessed word satisfies every check —, cost [B] int32: the quantised
        discrepancy of x to ``metric``, pattern [B] int32: the winning candidate's index, -1 for a word passed through)."""
        B, span = check_decode_osd_args(rel, metric, viol, self.N, order, span)
        _, row_ptr, _, row_var, N, M, E = self._device_tables('osd')
        rel = llr_batch(rel, self.device, N)
        metric = None if metric is None else llr_batch(metric, self.device, N)
        viol = None if viol is None else viol.to(self.device).contiguous()
        x = torch.empty((B, N), device=self.device, dtype=torch.uint8)
        cost, pattern = (torch.empty((B,), device=self.device, dtype=torch.int32) for _ in range(2))
        _hip.call('fgnn_ldpc_osd', rel, rel.stride(0) if B else N, metric, metric.stride(0) if B and metric is not None else N, viol,
                  row_ptr, row_var, B, N, M, E, int(order), span, x, cost, pattern)
        return x, cost, pattern


class Decoder(typing.NamedTuple):
    """A parsed classical decoder (``parse_decoder``'s result): its canonical spec, its kind ('mackay', 'llr', 'lp' or 'learned') and
    the arguments of that kind's decoder call."""
    spec: str
    kind: str
    args: dict

    def run(self, path, y, snr0):
        """Hard decisions, violated checks and iterations on received words y [B, N] at snr0 [B] dB, through ``path`` (an
        ``LdpcDataPath``).  A learned decoder's checkpoint is loaded on the first call and kept on ``path`` (once per checkpoint
        path); one trained for another code than ``path.code`` is refused (``LdpcCode.check_checkpoint``)."""
        return self.run_flags(path, y, snr0)[:3]

    @property
    def certifies(self):
        """Whether flag bit 1 of ``run_flags`` proves a word maximum-likelihood: the plain LP (kind 'lp', penalty 0)."""
        return self.kind == 'lp' and self.args['penalty'] == 0

    def run_flags(self, path, y, snr0):
        """``run``'s triple and, fourth, the decoder's own flags [B] int32 (``LdpcDecoders.decode_lp``'s: before any reprocessing) for
        kind 'lp', None for every other kind."""
        if self.kind == 'mackay':
            return path.decode(path.bit_prior(y, snr0), **self.args) + (None,)
        llr = path.bit_llr(y, snr0)
        if self.kind == 'learned':
            return tuple(path.learned(self.args['path']).decode(llr)) + (None,)
        if self.kind == 'lp':
            lp = dict(self.args)
            order, span = lp.pop('osd', None), lp.pop('span', None)
            if order is None:
                return path.decode_lp(llr, **lp)
            # ADMM-OSD: the words left with violated checks are reprocessed, ordered by |0.5 - x| and scored against the channel LLRs
            _, viol, iters, flags, soft = path.decode_lp(llr, want_soft=True, **lp)
            x = path.decode_osd(0.5 - soft, metric=llr, viol=viol, order=order, span=span)[0]
            return x, torch.zeros_like(viol), iters, flags
        if 'osd' in self.args:  # BP-OSD: the words the decoder leaves with violated checks are reprocessed against the channel LLRs
            bp = dict(self.args)
            order, span = bp.pop('osd'), bp.pop('span', None)
            _, viol, iters, post = path.decode_llr(llr, want_posteriors=True, **bp)
            x = path.decode_osd(post, metric=llr, viol=viol, order=order, span=span)[0]
            return x, torch.zeros_like(viol), iters, None
        return path.decode_llr(llr, **self.args) + (None,)


def parse_decoder(spec):
    """A classical decoder's spec -> (canonical spec, kind, arguments).  ``'mackay'``: the reference's probability-domain sum-product
    (``LdpcDataPath.decode``, 100 loops; ``mackay:iters=N`` for another count), kind 'mackay', arguments {'loops'}.  Otherwise
    ``ALGORITHM[:SCHEDULE][:iters=N][:alpha=A][:beta=B][:osd=W[:span=L]]`` with ALGORITHM 'min-sum', 'offset-min-sum' or
    'sum-product' and SCHEDULE 'flooding' (the default) or 'layered': kind 'llr', the keyword arguments of ``LdpcDataPath.decode_llr``.  The canonical spec
    names the schedule and then only what differs from the defaults, in the order iters, alpha, beta; parsing it gives itself.
    The LLR-domain specs take two more options behind ``beta``: ``osd=W`` (0..2) runs ordered-statistics reprocessing of order W on
    the words the decoder leaves with violated checks (``LdpcDataPath.decode_osd``), and ``span=L`` (>= 1; needs osd >= 1; at most
    256 with osd=2) bounds the positions it flips; the arguments then hold 'osd' (and 'span'), and the canonical spec appends them in
    that order.
    ``learned-min-sum:CHECKPOINT``: the trained min-sum decoder of an ``ldpc_nms_train`` checkpoint (``ldpc_nms.LearnedMinSum``), kind
    'learned', arguments {'path'}; everything behind the first colon is the path (it may hold colons), and the spec is canonical as
    it stands.
    ``admm-lp[:iters=N][:mu=M][:penalty=A][:relax=R][:eps=E][:osd=W[:span=L]]``: the ADMM linear-programming decoder
    (``LdpcDecoders.decode_lp``), kind 'lp', its keyword arguments max_iter, mu, penalty, relax and eps (defaults ``LP_DEFAULTS``;
    stop_on_codeword stays at its default, penalty > 0) and 'osd' / 'span' as above (the reprocessing orders by |0.5 - x|); the
    canonical spec lists only what differs from the defaults, in that order.  The triple is a ``Decoder``: ``.run(path, y, snr0)`` decodes with it."""
    if not isinstance(spec, str) or not spec:
        raise ValueError('a decoder spec is a non-empty string, got %r' % (spec,))
    if spec == LEARNED or spec.startswith(LEARNED + ':'):
        ckpt = spec[len(LEARNED) + 1:]
        if not ckpt:
            raise ValueError('decoder spec %r: %s:CHECKPOINT needs the path of a checkpoint' % (spec, LEARNED))
        return Decoder(spec, 'learned', {'path': ckpt})
    head, *rest = spec.split(':')
    if head == LP:
        return _parse_lp(spec, rest)
    opts, schedule = {}, None
    for part in rest:
        if part in LLR_SCHEDULES and schedule is None and not opts:
            schedule = part
            continue
        key, eq, val = part.partition('=')
        if not eq or key not in ('iters', 'alpha', 'beta', 'osd', 'span') or key in opts:
            raise ValueError('decoder spec %r: cannot read %r (SCHEDULE, iters=N, alpha=A, beta=B, osd=W, span=L)' % (spec, part))
        try:
            opts[key] = int(val) if key in ('iters', 'osd', 'span') else float(val)
        except ValueError:
            raise ValueError('decoder spec %r: %s=%r is not a number' % (spec, key, val)) from None
        if not (opts[key] >= (1 if key in ('iters', 'span') else 0)) or opts[key] > (OSD_MAX_ORDER if key == 'osd' else 3.0e38):
            raise ValueError('decoder spec %r: %s=%r is out of range' % (spec, key, val))
    if head == 'mackay':
        if schedule is not None or set(opts) - {'iters'}:
            raise ValueError('decoder spec %r: mackay takes iters=N only' % spec)
        loops = opts.get('iters', 100)
        return Decoder('mackay' + (':iters=%d' % loops if loops != 100 else ''), 'mackay', {'loops': loops})
    if head not in LLR_ALGORITHMS:
        raise ValueError('decoder spec %r: unknown decoder %r (mackay, %s)' % (spec, head, ', '.join(LLR_ALGORITHMS)))
    if 'alpha' in opts and head != 'min-sum' or 'beta' in opts and head != 'offset-min-sum':
        raise ValueError('decoder spec %r: alpha belongs to min-sum, beta to offset-min-sum' % spec)
    kw = {'algorithm': head, 'schedule': schedule or 'flooding', 'max_iter': opts.get('iters', 50), 'alpha': opts.get('alpha', 0.8125),
          'beta': opts.get('beta', 0.5)}
    canon = '%s:%s' % (head, kw['schedule'])
    canon += ':iters=%d' % kw['max_iter'] if kw['max_iter'] != 50 else ''
    canon += ':alpha=%r' % kw['alpha'] if kw['alpha'] != 0.8125 else ''
    canon += ':beta=%r' % kw['beta'] if kw['beta'] != 0.5 else ''
    if 'span' in opts and (opts.get('osd', 0) < 1 or opts['span'] >= 2 ** 31 or opts['osd'] == 2 and opts['span'] > OSD_MAX_PAIR_SPAN):
        raise ValueError('decoder spec %r: span=L needs osd=1 or osd=2 (then L <= %d)' % (spec, OSD_MAX_PAIR_SPAN))
    for key in ('osd', 'span'):
        if key in opts:
            kw[key] = opts[key]
            canon += ':%s=%d' % (key, opts[key])
    return Decoder(canon, 'llr', kw)


def _parse_lp(spec, parts):
    """``parse_decoder`` for an ``admm-lp`` spec; ``parts``: what follows the head."""
    keys = {'iters': 'max_iter', 'mu': 'mu', 'penalty': 'penalty', 'relax': 'relax', 'eps': 'eps', 'osd': 'osd', 'span': 'span'}
    opts = {}
    for part in parts:
        key, eq, val = part.partition('=')
        if not eq or key not in keys or key in opts:
            raise ValueError('decoder spec %r: cannot read %r (iters=N, mu=M, penalty=A, relax=R, eps=E, osd=W, span=L)' % (spec, part))
        try:
            opts[key] = int(val) if key in ('iters', 'osd', 'span') else float(val)
        except ValueError:
            raise ValueError('decoder spec %r: %s=%r is not a number' % (spec, key, val)) from None
        v = opts[key]
        ok = {'iters': 1 <= v < 2 ** 31, 'span': 1 <= v < 2 ** 31, 'osd': 0 <= v <= OSD_MAX_ORDER, 'mu': 0 < v <= 3.0e38,
              'relax': 1 <= v < 2, 'eps': abs(v) <= 3.0e38}.get(key, 0 <= v <= 3.0e38)
        if not ok:
            raise ValueError('decoder spec %r: %s=%r is out of range' % (spec, key, val))
    if 'span' in opts and (opts.get('osd', 0) < 1 or opts['osd'] == 2 and opts['span'] > OSD_MAX_PAIR_SPAN):
        raise ValueError('decoder spec %r: span=L needs osd=1 or osd=2 (then L <= %d)' % (spec, OSD_MAX_PAIR_SPAN))
    kw, canon = dict(LP_DEFAULTS), LP
    for key in ('iters', 'mu', 'penalty', 'relax', 'eps'):
        if key in opts and opts[key] != LP_DEFAULTS[keys[key]]:
            kw[keys[key]] = opts[key]
            canon += ':%s=%s' % (key, '%d' % opts[key] if key == 'iters' else repr(opts[key]))
    for key in ('osd', 'span'):
        if key in opts:
            kw[key] = opts[key]
            canon += ':%s=%d' % (key, opts[key])
    return Decoder(canon, 'lp', kw)
