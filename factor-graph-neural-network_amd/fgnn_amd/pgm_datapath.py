"""The synthetic-PGM data path, per batch on the GPU: the reference's random chain models and their exact MAP labels.

The reference makes the datasets of train_syn_pw_factor.py / train_syn_hop_factor.py on the host, one item at a time
(/root/reference/lib/data/random_pgm.py, random_pgm_pw.py, random_pgm_hop.py and the NoHop variants; written to a pickle stream
by data_generate/generate_random_pgm.py), and labels every item with AD3's branch-and-bound.  Those models are chains of binary
variables with 2x2 link factors and a budget factor on every window of h consecutive variables, so the exact MAP is a Viterbi
recursion over the last h-1 bits.  ``PgmDataPath`` runs that recursion (csrc/pgm_datapath.hip, one wave64 per sample) on
potentials the caller has (``solve_map``) or on models it draws itself (``sample``).

The reference labels every item a second time, with the argmax of AD3's LP-relaxation posteriors (``assign1``, the ``lp_acc``
baseline of train_syn_*.py).  ``solve_lp`` solves that LP the way AD3 does, by ADMM over the local polytope (csrc/pgm_lp.hip, one
wave64 per sample, f64), from AD3's start with its default step, tolerance and iteration cap; ``sample(..., lp_label=True)`` and
``write_reference_dataset(..., lp_label=True)`` add that label.

``solve_bp`` is the baseline the network is named after, which the reference does not have: damped parallel max-product belief
propagation on the same chains (csrc/pgm_bp.hip, one wave64 per sample, f64, messages in LDS); ``sample(..., bp_label=True)`` adds
its label.  No CPU fallback.
"""
import ctypes
import pickle

import numpy as np
import torch

from . import _hip

FAMILIES = {'raw': 0, 'pws': 1, 'hops': 2}


def check_chain(N, h):
    """ValueError unless the solver takes chains of N variables with windows of h (2 <= h <= 13, N >= h, the per-sample LDS
    footprint within the workgroup limit).  Asks the library (fgnn_chain_budget_map_lds_bytes), no device needed."""
    N, h = int(N), int(h)
    L = _hip.lib()
    if L.fgnn_chain_budget_map_lds_bytes(N, h) < 0:
        raise ValueError(L.fgnn_last_error().decode())
    return N, h


def _batched(t, name, per_sample, B=None):
    """t of shape per_sample (shared: batch stride 0) or [B] + per_sample -> (tensor with a batch axis, batch size or None)."""
    per_sample = tuple(per_sample)
    if tuple(t.shape) == per_sample:
        return t.unsqueeze(0), None
    if t.dim() == len(per_sample) + 1 and tuple(t.shape[1:]) == per_sample and (B is None or t.shape[0] == B):
        return t, t.shape[0]
    raise ValueError('%s must be %s or [B, %s]%s, got %s' % (name, list(per_sample), ', '.join(map(str, per_sample)),
                                                            '' if B is None else ' with B = %d' % B, tuple(t.shape)))


def check_solve_args(unary, pair, caps, N, h):
    """Shapes of a ``solve_map`` call, checked before anything reaches the device.  unary [B,N,2]; pair [N-1,4] / [N-1,2,2] or with
    a leading [B]; caps an int, [N-h+1] or [B,N-h+1].  Returns (B, unary, pair [*,N-1,4], caps [*,N-h+1]) as tensors."""
    N, h = check_chain(N, h)
    unary = torch.as_tensor(unary)
    if unary.dim() != 3 or tuple(unary.shape[1:]) != (N, 2):
        raise ValueError('unary must be [B, %d, 2], got %s' % (N, tuple(unary.shape)))
    B = unary.shape[0]
    pair = torch.as_tensor(pair)
    if pair.shape[-2:] == (2, 2):
        pair = pair.reshape(tuple(pair.shape[:-2]) + (4,))
    pair, _ = _batched(pair, 'pair', (N - 1, 4), B)
    if isinstance(caps, (int, np.integer)):
        caps = torch.full((N - h + 1,), int(caps), dtype=torch.int32)
    caps = torch.as_tensor(caps)
    if caps.is_floating_point() or caps.is_complex() or caps.dtype == torch.bool:
        raise ValueError('caps must be integers, got %s' % caps.dtype)
    caps, _ = _batched(caps, 'caps', (N - h + 1,), B)
    return B, unary, pair, caps


def check_bp_args(N, h, max_iter=200, damping=0.5, tol=1e-6):
    """ValueError unless ``solve_bp`` takes these: a shape within the kernel's LDS (fgnn_chain_budget_bp_lds_bytes), max_iter >= 0,
    damping in [0, 1), tol finite and >= 0.  No device needed.  Returns (max_iter, damping, tol) as int, float, float."""
    L = _hip.lib()
    if _hip.invoke('fgnn_chain_budget_bp_lds_bytes', int(N), int(h)) < 0:
        raise ValueError(L.fgnn_last_error().decode())
    max_iter, damping, tol = int(max_iter), float(damping), float(tol)
    if max_iter < 0:
        raise ValueError('max_iter must be >= 0, got %d' % max_iter)
    if not 0 <= damping < 1:
        raise ValueError('damping must be in [0, 1), got %r' % damping)
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError('tol must be a finite value >= 0, got %r' % tol)
    return max_iter, damping, tol


class PgmDataPath:
    """Chains of ``chain_length`` binary variables with budget windows of ``hop_order`` (the reference's 30 and 9).

    ``solve_map`` labels potentials the caller has; ``sample`` draws a training batch of the reference's models (families
    ``raw`` = RandomPGM, ``pws`` = RandomPGMPw, ``hops`` = RandomPGMHop) and labels it; ``write_reference_dataset`` writes the
    reference's pickle stream for an unchanged ``train_syn_*.py --train_path``."""

    def __init__(self, device, chain_length=30, hop_order=9):
        self.N, self.h = check_chain(chain_length, hop_order)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('PgmDataPath runs on a ROCm device (no CPU fallback)')

    def solve_map(self, unary, pair, caps, want_objective=False):
        """Exact MAP of B chains: unary [B,N,2] log-potentials; pair [N-1,4] (row-major [x_i][x_{i+1}], or [N-1,2,2]) or
        [B,N-1,4]; caps: an int, [N-h+1] or [B,N-h+1] — window w = x_w .. x_{w+h-1} holds at most caps[w] ones (cap >= h: no
        constraint, the NoHop models).  Potentials are read as f32 and summed in f64.  Ties: the lowest state (csrc/pgm_datapath.hip).
        Returns labels [B,N] int64 (and the objective [B] f64 with want_objective)."""
        B, unary, pair, caps = check_solve_args(unary, pair, caps, self.N, self.h)
        dev = self.device
        if B == 0:
            labels = torch.empty((0, self.N), device=dev, dtype=torch.int64)
            return (labels, torch.empty((0,), device=dev, dtype=torch.float64)) if want_objective else labels
        u = unary.to(dev, torch.float32).contiguous()
        p = pair.to(dev, torch.float32).contiguous()
        c = caps.to(dev, torch.int32).contiguous()
        sb = lambda t: 0 if t.shape[0] == 1 and B != 1 else t[0].numel()
        labels = torch.empty((B, self.N), device=dev, dtype=torch.int64)
        obj = torch.empty((B,), device=dev, dtype=torch.float64) if want_objective else None
        _hip.call('fgnn_chain_budget_map', u, u[0].numel(), p, sb(p), c, sb(c), B, self.N, self.h, labels, obj)
        return (labels, obj) if want_objective else labels

    def solve_lp(self, unary, pair, caps, max_iter=1000, tol=1e-6, eta=0.1, adapt=True, want_details=False):
        """The LP relaxation of the same B chains (inputs as ``solve_map``), by AD3-style ADMM (csrc/pgm_lp.hip): start z = 1/2,
        step ``eta`` with residual balancing every 50th iteration when ``adapt``, stop when both RMS residuals are below ``tol`` or
        after ``max_iter`` iterations (the defaults are the reference's call, AD3's ``solve()`` defaults).  Returns labels [B,N]
        int64 (z_i > 0.5; ties to 0), and with want_details also a dict of marginals [B,N] f64 (z), value [B] f64 (the LP
        objective at z), status [B] int32 (0 integral, 1 fractional, 2 infeasible: a negative cap, 3 iteration cap reached) and
        iters [B] int32."""
        B, unary, pair, caps = check_solve_args(unary, pair, caps, self.N, self.h)
        max_iter, tol, eta = int(max_iter), float(tol), float(eta)
        if max_iter < 0:
            raise ValueError('max_iter must be >= 0, got %d' % max_iter)
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError('tol must be a finite value >= 0, got %r' % tol)
        if not (np.isfinite(eta) and eta > 0):
            raise ValueError('eta must be a finite value > 0, got %r' % eta)
        dev, N = self.device, self.N
        labels = torch.empty((B, N), device=dev, dtype=torch.int64)
        det = dict(marginals=torch.empty((B, N), device=dev, dtype=torch.float64),
                   value=torch.empty((B,), device=dev, dtype=torch.float64),
                   status=torch.empty((B,), device=dev, dtype=torch.int32),
                   iters=torch.empty((B,), device=dev, dtype=torch.int32)) if want_details else None
        if B > 0:
            u = unary.to(dev, torch.float32).contiguous()
            p = pair.to(dev, torch.float32).contiguous()
            c = caps.to(dev, torch.int32).contiguous()
            sb = lambda t: 0 if t.shape[0] == 1 and B != 1 else t[0].numel()
            d = det or {}
            _hip.call('fgnn_chain_budget_lp', u, u[0].numel(), p, sb(p), c, sb(c), B, N, self.h, max_iter, tol, eta, 1 if adapt else 0,
                      labels, d.get('marginals'), d.get('value'), d.get('status'), d.get('iters'))
        return (labels, det) if want_details else labels

    def solve_bp(self, unary, pair, caps, max_iter=200, damping=0.5, tol=1e-6, want_details=False):
        """Max-product belief propagation on the same B chains (inputs as ``solve_map``), csrc/pgm_bp.hip: messages as log-ratios in
        f64, all 0 at the start, all updated in parallel, ``new = damping * old + (1 - damping) * computed``; a sample stops after
        the iteration whose largest message change is below ``tol`` (strict: tol = 0 runs ``max_iter`` iterations) or after
        ``max_iter``.  On these loopy graphs (overlapping windows) it is a heuristic; with every cap >= h the graph is a chain and
        ``max_iter=N, damping=0`` gives the exact MAP.  Returns labels [B,N] int64 (1 where the final belief is > 0), and with
        want_details also a dict of beliefs [B,N] f64, status [B] int32 (0 converged, 2 a negative cap: labels and beliefs 0, 3
        iteration cap reached) and iters [B] int32."""
        B, unary, pair, caps = check_solve_args(unary, pair, caps, self.N, self.h)
        max_iter, damping, tol = check_bp_args(self.N, self.h, max_iter, damping, tol)
        dev, N = self.device, self.N
        labels = torch.empty((B, N), device=dev, dtype=torch.int64)
        det = dict(beliefs=torch.empty((B, N), device=dev, dtype=torch.float64),
                   status=torch.empty((B,), device=dev, dtype=torch.int32),
                   iters=torch.empty((B,), device=dev, dtype=torch.int32)) if want_details else None
        if B > 0:
            u = unary.to(dev, torch.float32).contiguous()
            p = pair.to(dev, torch.float32).contiguous()
            c = caps.to(dev, torch.int32).contiguous()
            sb = lambda t: 0 if t.shape[0] == 1 and B != 1 else t[0].numel()
            d = det or {}
            _hip.call('fgnn_chain_budget_bp', u, u[0].numel(), p, sb(p), c, sb(c), B, N, self.h, max_iter, tol, damping, labels,
                      d.get('beliefs'), d.get('status'), d.get('iters'))
        return (labels, det) if want_details else labels

    def lp_inputs(self, family, sampled, cap=5, transition=(0, .1, .2, 1)):
        """The (unary [B,N,2], pair, caps) of models ``sample(..., family)`` drew, rebuilt on the device from its output tuple:
        unary = node feature transposed; pair = the pws feature's to-right link ([B,N-1,4]) or the shared ``transition``; caps = the
        hop feature's one-hot at position w + h/2 ([B,N-h+1]) or ``cap``."""
        N, h, dev = self.N, self.h, self.device
        unary = sampled[0][:, :, :, 0].transpose(1, 2)
        if family == 'raw':
            pair = torch.tensor([float(v) for v in transition], dtype=torch.float32, device=dev).expand(N - 1, 4)
        else:
            pair = sampled[1][:, :, :N - 1, 0].transpose(1, 2)
        if family == 'hops':
            caps = sampled[2][:, :, h // 2:h // 2 + N - h + 1, 0].argmax(1).to(torch.int32)
        else:
            caps = int(cap)
        return unary, pair, caps

    def sample(self, B, family='hops', seed=0, step=0, cap=5, transition=(0, .1, .2, 1), want_objective=False, lp_label=False,
               bp_label=False):
        """One training batch of B random models, drawn in the kernel from (seed, step) (Philox4x32-10; a training loop passes its
        step), in the tuple order the reference's ``RandomPGMData`` yields for ``family``:
          hops: (node_feature [B,2,N,1], pws [B,4,N,1], hops [B,h,N,1], label [B,N])   RandomPGMHop (per-position caps)
          pws:  (node_feature, pws, label)                                             RandomPGMPw (every window ``cap``)
          raw:  (node_feature, label)                                                  RandomPGM (link table ``transition``)
        Features f32, labels int64 = the exact MAP.  ``cap`` >= h gives the NoHop variants.  With lp_label the LP-relaxation label
        [B,N] int64 of ``solve_lp`` at its defaults follows the MAP label (the reference's (..., assign, assign1)); with
        bp_label the max-product label [B,N] int64 of ``solve_bp`` at its defaults follows those; with want_objective the MAP
        objective [B] f64 is appended last."""
        if family not in FAMILIES:
            raise ValueError('family must be one of %s, got %r' % (sorted(FAMILIES), family))
        B = int(B)
        if B < 0:
            raise ValueError('batch must be >= 0')
        if len(tuple(transition)) != 4:
            raise ValueError('transition must hold 4 values (row-major [x_i][x_{i+1}])')
        N, h, dev = self.N, self.h, self.device
        if bp_label:
            check_bp_args(N, h)
        fam = FAMILIES[family]
        node = torch.empty((B, 2, N, 1), device=dev, dtype=torch.float32)
        pws = torch.empty((B, 4, N, 1), device=dev, dtype=torch.float32) if fam != 0 else None
        hops = torch.empty((B, h, N, 1), device=dev, dtype=torch.float32) if fam == 2 else None
        label = torch.empty((B, N), device=dev, dtype=torch.int64)
        obj = torch.empty((B,), device=dev, dtype=torch.float64) if want_objective else None
        trans = (ctypes.c_float * 4)(*[float(v) for v in transition])          # host memory, copied into the launch
        _hip.call('fgnn_pgm_sample_rng', fam, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, B, N, h, int(cap), trans,
                  node, pws, hops, label, obj)
        out = (node, pws, hops, label) if fam == 2 else (node, pws, label) if fam == 1 else (node, label)
        if lp_label:
            out = out + (self.solve_lp(*self.lp_inputs(family, out, cap, transition)),)
        if bp_label:
            out = out + (self.solve_bp(*self.lp_inputs(family, out, cap, transition)),)
        return out + (obj,) if want_objective else out

    def write_reference_dataset(self, path, family, size, seed, step=0, batch=4096, cap=5, transition=(0, .1, .2, 1),
                                lp_label=False):
        """Write ``size`` items of ``family`` as the reference's pickle stream (data_generate/generate_random_pgm.py: one
        ``pickle.dump`` per item), readable by ``RandomPGMData(path, family, size)`` and so by an unchanged
        ``train_syn_*.py --train_path``.  Items come from ``sample(batch, family, seed, step + k)`` for k = 0, 1, ..., so item i of
        the first chunk is item i of ``sample(..., seed, step)``.  Per item, as random_pgm*.py returns them with the features
        unexpanded: hops (node_feature [2,N], pws [4,N,1], hop feature [h,N,1] f32, assign [N], assign1 [N] int64), pws
        (node_feature, pws, assign, assign1), raw (node_feature, assign, assign1).

        ``assign`` is the exact MAP.  ``assign1`` is the reference's label from AD3's LP relaxation (``solve(branch_and_bound=False)``):
        with lp_label, ``solve_lp``'s label at its defaults (the same LP, solved from AD3's start with its defaults; where the LP
        optimum is not unique or the iteration cap is reached it may differ from what AD3 would return); without, it is -1
        everywhere and the scripts' ``lp_acc`` reads 0."""
        size, batch = int(size), max(1, int(batch))
        with open(path, 'wb') as f:
            k = 0
            while k * batch < size:
                n = min(batch, size - k * batch)
                out = [t.cpu().numpy() for t in self.sample(n, family, seed, step + k, cap, transition, lp_label=lp_label)]
                if lp_label:
                    lp = out.pop()
                else:
                    lp = np.full((n, self.N), -1, np.int64)
                label = out[-1]
                feats = [np.ascontiguousarray(out[0][:, :, :, 0])] + out[1:-1]                  # node_feature [2,N]; pws / hops keep their [.., N, 1]
                for i in range(n):
                    pickle.dump(tuple(a[i] for a in feats) + (label[i], lp[i].copy()), f)
                k += 1
