"""Learned ("neural") min-sum LDPC decoding: a flooding or layered min-sum whose normalisation weights ``alpha`` and offsets ``beta``
are trained (Nachmani et al.'s neural min-sum, Lugosch & Gross's neural offset min-sum) — the learned decoder FGNN's papers compare
against.

The reference has no counterpart.  The decoder is defined in include/fgnn_hip_ldpc_nms.h: ``n_iter`` flooding iterations, in iteration
t every check sends ``s * max(alpha_t[w] * mag - beta_t[w], 0)`` with ``mag`` the smallest |q| among the other edges, and the weights
are shared per iteration, per (iteration, check) or per (iteration, edge).  Forward and backward are the two kernels of
csrc/ldpc_nms.hip; there is no torch fallback.  ``schedule='layered'`` runs the same check update layer by layer
(``LdpcCode.layers()``), each check on the totals the earlier layers of the iteration left: include/fgnn_hip_ldpc_nms_layered.h,
the two kernels of csrc/ldpc_nms_layered.hip.  It takes every code ``LdpcCode.require_llr_decoder`` takes (csrc/ldpc_word.h's
limits: N, M <= 1024, degrees <= 16).

    dec = LearnedMinSum(code, n_iter=5, share='edge').cuda()          # schedule='layered': the layered decoder
    totals = dec(llr)                         # [n_iter, B, N]: every iteration's totals, differentiable in alpha, beta and llr
    multi_loss(totals, cw).backward()
    x, viol, iters = dec.decode(llr)          # early stopping, no gradient

``python -m fgnn_amd.ldpc_nms_train`` trains one; ``python -m fgnn_amd.ldpc_eval --decoder learned-min-sum:CHECKPOINT`` evaluates it.
"""
import numpy as np
import torch

from . import _hip
from .ldpc_code import LdpcCode
from .ldpc_decoders import LEARNED as KIND, check_word_batch, decode_outputs, llr_batch   # KIND: a checkpoint's decoder['kind']

SHARES = {'iteration': 0, 'check': 1, 'edge': 2}       # fgnn_ldpc_nms_forward's ``share``
MAX_ITER = 64                                          # csrc/ldpc_nms.h's NMS_MAXIT
SCHEDULES = ('flooding', 'layered')


def check_nms_args(llr, n_var, n_chk, n_edges, n_iter, share, alpha, beta):
    """Arguments of ``LearnedMinSum.forward`` / ``decode`` (before anything reaches the device): llr [B, n_var] floating point,
    ``n_iter`` an integer in 1..64, ``share`` one of ``SHARES``, alpha and beta f32 tensors [n_iter, W] with W = 1, n_chk or n_edges.
    Returns (B, the share's code, W)."""
    W = weights_per_iteration(n_iter, share, n_chk, n_edges)
    for what, v in (('alpha', alpha), ('beta', beta)):
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != (int(n_iter), W):
            raise ValueError('%s must be a float32 tensor [%d, %d], got %s' % (
                what, n_iter, W, '%s %s' % (v.dtype, tuple(v.shape)) if isinstance(v, torch.Tensor) else type(v).__name__))
    return check_word_batch('llr', llr, n_var), SHARES[share], W


def weights_per_iteration(n_iter, share, n_chk, n_edges):
    """W of alpha / beta [n_iter, W]; refuses an ``n_iter`` outside 1..64 and an unknown ``share``."""
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or not 1 <= int(n_iter) <= MAX_ITER:
        raise ValueError('n_iter must be an integer in 1..%d, got %r' % (MAX_ITER, n_iter))
    if not isinstance(share, str) or share not in SHARES:
        raise ValueError('share must be one of %s, got %r' % (', '.join(SHARES), share))
    return (1, int(n_chk), int(n_edges))[SHARES[share]]


def backward_workgroups(B):
    """The number of workgroups ``fgnn_ldpc_nms_backward`` launches over B words (workgroup g takes the words g, g + G, ...)."""
    return int(_hip.invoke('fgnn_ldpc_nms_backward_workgroups', int(B)))


def _query(name, *args):
    r = int(_hip.invoke(name, *args))
    if r < 0:
        raise _hip.FgnnHipError('libfgnn_hip: %s' % _hip.lib().fgnn_last_error().decode())
    return r


def _entry_point(which, tables, layers):
    """(the name of the forward / backward entry point, its table arguments): ``layers`` = None for the flooding schedule, else the
    device tensors (layer_ptr, layer_chk)."""
    if layers is None:
        return 'fgnn_ldpc_nms_' + which, tuple(tables)
    return 'fgnn_ldpc_nms_layered_' + which, tuple(tables) + (layers[0], layers[1], layers[0].numel() - 1)


def nms_forward_raw(llr, tables, sizes, alpha, beta, n_iter, share, layers=None):
    """The train-mode launch: (totals [n_iter, B, N] f32, record uint8 [record bytes]).  llr [B, N] f32 on the device, unit column
    stride.  ``layers``: None, or (layer_ptr, layer_chk) for the layered schedule."""
    N, M, E = sizes
    B = llr.shape[0]
    totals = torch.empty((n_iter, B, N), device=llr.device, dtype=torch.float32)
    nbytes = _query('fgnn_ldpc_nms_record_bytes', B, N, M, E, n_iter)
    record = torch.empty((nbytes,), device=llr.device, dtype=torch.uint8)
    name, tabs = _entry_point('forward', tables, layers)
    _hip.call(name, llr, llr.stride(0) if B else N, *tabs, alpha, beta, B, N, M, E, n_iter, share, 0, None, None, None, None, totals,
              record, nbytes)
    return totals, record


def nms_backward_raw(g_totals, llr, tables, sizes, alpha, beta, record, n_iter, share, want_llr=True, layers=None):
    """The backward's two launches: (g_alpha, g_beta [n_iter, W] f32, g_llr [B, N] f32 or None).  g_totals [n_iter, B, N], any
    strides (the kernel reads it densely: a strided one is copied).  ``layers`` as the forward's that wrote ``record``."""
    N, M, E = sizes
    B = llr.shape[0]
    if tuple(g_totals.shape) != (n_iter, B, N):
        raise ValueError('g_totals must be [%d, %d, %d], got %s' % (n_iter, B, N, tuple(g_totals.shape)))
    g_totals = g_totals.to(torch.float32).contiguous()
    g_alpha, g_beta = torch.empty_like(alpha), torch.empty_like(beta)
    g_llr = torch.empty((B, N), device=llr.device, dtype=torch.float32) if want_llr else None
    nbytes = _query('fgnn_ldpc_nms_backward_workspace_bytes', B, N, M, E, n_iter, share)
    ws = torch.empty((max(nbytes, 16),), device=llr.device, dtype=torch.uint8)
    name, tabs = _entry_point('backward', tables, layers)
    _hip.call(name, g_totals, llr, llr.stride(0) if B else N, *tabs, alpha, beta, record, record.numel(), B, N, M, E, n_iter, share,
              g_alpha, g_beta, g_llr, ws, ws.numel())
    return g_alpha, g_beta, g_llr


class _NmsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, llr, alpha, beta, tables, sizes, n_iter, share, layers):
        alpha, beta = alpha.detach().contiguous(), beta.detach().contiguous()
        totals, record = nms_forward_raw(llr, tables, sizes, alpha, beta, n_iter, share, layers)
        ctx.save_for_backward(llr, alpha, beta, record)
        ctx.nms = (tables, sizes, n_iter, share, layers)
        return totals

    @staticmethod
    def backward(ctx, g_totals):
        llr, alpha, beta, record = ctx.saved_tensors
        tables, sizes, n_iter, share, layers = ctx.nms
        g_alpha, g_beta, g_llr = nms_backward_raw(g_totals, llr, tables, sizes, alpha, beta, record, n_iter, share,
                                                  want_llr=ctx.needs_input_grad[0], layers=layers)
        return g_llr, g_alpha, g_beta, None, None, None, None, None


class LearnedMinSum(torch.nn.Module):
    """Min-sum with trained weights for ``code`` (an ``LdpcCode`` within ``require_llr_decoder``'s limits; None: the built-in
    96.3.963): parameters ``alpha`` and ``beta`` [n_iter, W] f32, W = 1 (``share='iteration'``), M ('check') or E ('edge', indexed by
    the edge id e = col_ptr[n] + u), filled with the constants ``alpha`` / ``beta``.  ``schedule``: 'flooding', or 'layered' over
    ``code.layers()``.  ``state_dict()`` is the two parameters; the incidence (and layer) tables are buffers outside it and follow
    ``.to(device)``.  The module runs on a ROCm device only."""

    def __init__(self, code=None, n_iter=5, share='edge', alpha=0.8125, beta=0.0, schedule='flooding'):
        super().__init__()
        code = LdpcCode.builtin() if code is None else code
        if not isinstance(code, LdpcCode):
            raise TypeError('code must be an LdpcCode or None, got %s' % type(code).__name__)
        code.require_llr_decoder()
        tabs = code.incidence_tables()
        self.N, self.M, self.E = code.n_var, code.n_chk, int(tabs[0][-1])
        W = weights_per_iteration(n_iter, share, self.M, self.E)
        if not isinstance(schedule, str) or schedule not in SCHEDULES:
            raise ValueError('schedule must be one of %s, got %r' % (', '.join(SCHEDULES), schedule))
        self.code, self.n_iter, self.share, self.schedule = code, int(n_iter), share, schedule
        for name, value in (('alpha', alpha), ('beta', beta)):
            if not np.isfinite(float(value)):
                raise ValueError('%s must be finite, got %r' % (name, value))
            self.register_parameter(name, torch.nn.Parameter(torch.full((self.n_iter, W), float(value))))
        for name, a in zip(('col_ptr', 'row_ptr', 'row_edge', 'row_var'), tabs):
            self.register_buffer(name, torch.from_numpy(a.copy()), persistent=False)
        if schedule == 'layered':
            for name, a in zip(('layer_ptr', 'layer_chk'), code.layers()):
                self.register_buffer(name, torch.from_numpy(a.copy()), persistent=False)

    def extra_repr(self):
        return '%r, n_iter=%d, share=%r%s' % (self.code, self.n_iter, self.share, ', schedule=%r' % self.schedule if self.schedule != 'flooding' else '')

    def decoder_entry(self):
        """What a checkpoint carries under 'decoder'; 'schedule' only where it is not flooding."""
        entry = {'kind': KIND, 'n_iter': int(self.n_iter), 'share': self.share}
        if self.schedule != 'flooding':
            entry['schedule'] = self.schedule
        return entry

    def layer_tables(self):
        """(layer_ptr, layer_chk) on the module's device for the layered schedule, None for flooding: the raw launches' ``layers``."""
        return (self.layer_ptr, self.layer_chk) if self.schedule == 'layered' else None

    def _prepare(self, llr):
        B, share, _ = check_nms_args(llr, self.N, self.M, self.E, self.n_iter, self.share, self.alpha, self.beta)
        if self.alpha.device.type != 'cuda':
            raise RuntimeError('LearnedMinSum runs on a ROCm device (no CPU fallback): move the module there first')
        return llr_batch(llr, self.alpha.device, self.N), B, share, (self.col_ptr, self.row_ptr, self.row_edge, self.row_var), (self.N, self.M, self.E)

    def forward(self, llr):
        """llr [B, N] = log P(bit = 0) / P(bit = 1) -> totals [n_iter, B, N] f32, every iteration's totals (no early stop), through
        the train mode of ``fgnn_ldpc_nms_forward`` (layered: ``fgnn_ldpc_nms_layered_forward``); differentiable in ``alpha``,
        ``beta`` and, where it asks for it, ``llr``."""
        llr, _, share, tables, sizes = self._prepare(llr)
        return _NmsFunction.apply(llr, self.alpha, self.beta, tables, sizes, int(self.n_iter), share, self.layer_tables())

    @torch.no_grad()
    def decode(self, llr, want_posteriors=False):
        """The decode mode (a word stops after the first iteration that leaves no violated check): (x [B, N] uint8 hard decisions —
        the message is x[:, :K] —, violated checks [B] int32, iterations [B] int32[, post [B, N] f32: the final totals])."""
        llr, B, share, tables, (N, M, E) = self._prepare(llr)
        x, post, viol, iters = decode_outputs(B, N, llr.device, torch.float32 if want_posteriors else None)
        name, tabs = _entry_point('forward', tables, self.layer_tables())
        _hip.call(name, llr, llr.stride(0) if B else N, *tabs, self.alpha.detach().contiguous(), self.beta.detach().contiguous(), B, N, M,
                  E, int(self.n_iter), share, 1, x, post, viol, iters, None, None, 0)
        return (x, viol, iters, post) if want_posteriors else (x, viol, iters)


def multi_loss(totals, cw):
    """The multi-loss of the neural decoders' papers: the mean over iterations, words and all N bits of
    ``binary_cross_entropy_with_logits(-totals, cw)`` (a total is log P(0) / P(1): the logit of bit = 1 is -T).  totals [n_iter, B,
    N], cw [B, N] (the transmitted codeword, any dtype)."""
    target = cw.to(totals.dtype).unsqueeze(0).expand_as(totals)
    return torch.nn.functional.binary_cross_entropy_with_logits(-totals, target)


def load_checkpoint(path, code=None, device='cpu'):
    """The ``LearnedMinSum`` of an ``ldpc_nms_train`` checkpoint for ``code`` (None: the built-in 96.3.963).  A checkpoint trained for
    another code, or one that holds no learned min-sum decoder, is refused with a ValueError."""
    code = LdpcCode.builtin() if code is None else code
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    entry = ckpt.get('decoder') if isinstance(ckpt, dict) else None
    if not isinstance(entry, dict) or entry.get('kind') != KIND:
        raise ValueError('%s holds no learned min-sum decoder (no \'decoder\' entry of kind %r)' % (path, KIND))
    code.check_checkpoint(ckpt, path)
    dec = LearnedMinSum(code, int(entry['n_iter']), entry['share'], schedule=entry.get('schedule', 'flooding'))
    dec.load_state_dict(ckpt['model_state_dict'], strict=True)
    return dec.to(device)
