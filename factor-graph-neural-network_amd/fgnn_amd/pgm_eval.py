"""Evaluating synthetic-PGM MAP models on the GPU: the reference's test loop, and how good the decisions are as MAP solutions.

The reference's synthetic scripts end in a test loop (/root/reference/train_syn_fixed_pw_hop.py:313-362,
train_syn_pw_factor.py:349-411, train_syn_hop_factor.py:349-409): the model in eval mode over a stored test set in batches of 32,
then ``acc`` and ``acc_lp`` (the mean of the per-batch accuracies of the model's argmax and of the LP-relaxation label against the
exact MAP label), their per-batch standard deviations and the cross-entropy loss.  Here the whole loop stays on the device:
``score`` (csrc/pgm_eval.hip, one launch per batch) counts the correct variables and the NLL of every sample, and it also scores
every decision against the model's potentials: is it feasible (every budget window holds), what is its objective, how far is that
from the MAP's.  The reference reports none of that; per-variable accuracy alone says little about MAP inference.

``evaluate(..., bp=True)`` adds the baseline the network is named after and the reference lacks: max-product belief propagation
(``PgmDataPath.solve_bp``, csrc/pgm_bp.hip), solved on the test set's potentials and scored like the LP label.

``load_test_set`` reads the reference's pickle stream (``RandomPGMData``'s item formats), ``make_test_set`` writes one,
``build_model`` / ``load_checkpoint`` rebuild the scripts' models and read their checkpoints, ``evaluate`` runs the loop and
``python -m fgnn_amd.pgm_eval`` is the command line.
"""
import argparse
import contextlib
import json
import math
import os
import pickle
import statistics
import sys

import numpy as np
import torch

from . import _hip
from .pgm_datapath import FAMILIES, PgmDataPath, check_bp_args, check_solve_args

TRANSITION = (0, .1, .2, 1)          # data_generate/generate_random_pgm.py: the raw family's link table
CAP = 5                              # ... and budget (raw, pws)
HOP_ORDER = 9                        # every script's --hop_order
TEST_STEP = 1 << 62                  # make_test_set's first Philox step: training loops use steps from 0, far below this
MODEL_NAMES = {'raw': ('mp_nn', 'mp_nn_comp', 'simple_gnn', 'iid'), 'pws': ('mp_nn_factor',), 'hops': ('mp_nn_factor',)}
EDGE_KEYS = {'raw': ('emodel_state_dict',), 'pws': ('emodel_pw_state_dict', 'emodel_high_state_dict'),
             'hops': ('emodel_pw_state_dict', 'emodel_high_state_dict')}
OPT_RTOL = 1e-9                      # a feasible decision within this relative distance of the MAP objective counts as optimal


def _check_family(family):
    if family not in FAMILIES:
        raise ValueError('family must be one of %s, got %r' % (sorted(FAMILIES), family))


def score(dec, label, unary, pair, caps, h=HOP_ORDER, counts=None, out=None):
    """Scores of B decisions on B chains of N = label.shape[1] binary variables, one launch (csrc/pgm_eval.hip).

    dec: logits [B, 2, N, 1] or [B, 2, N] f32 / bf16, read through their strides (a model's output as it is), decision = 1 exactly
    when ``torch.argmax`` over the two classes returns 1 (ties and a NaN class 0 give 0); or assignments [B, N] int64 (x = a != 0).
    label [B, N] int64, the exact MAP.  unary, pair, caps as ``PgmDataPath.solve_map`` takes them (checked by ``check_solve_args``).
    Returns a dict of device tensors: correct [B] int32 (variables equal to the label), feasible [B] bool (every window within its
    cap), objective [B] f64 (the log-potential sum, in the MAP recursion's order: the MAP label scores ``solve_map``'s objective) and,
    for logits, nll [B] f64 (the sum of ``F.cross_entropy``'s summands).  ``counts`` [4] int64, if given, is ADDED to: variables
    compared, variables correct, feasible samples, samples equal to the label everywhere.  ``out``: preallocated outputs (the dict's
    keys, each a [B] tensor of the dtype above, feasible as uint8) to write into instead."""
    if label.dim() != 2 or label.dtype != torch.int64:
        raise ValueError('label must be [B, N] int64, got %s %s' % (tuple(label.shape), label.dtype))
    B, N = label.shape
    B2, unary, pair, caps = check_solve_args(unary, pair, caps, N, h)
    if B2 != B:
        raise ValueError('unary has %d samples, label %d' % (B2, B))
    if dec.dtype in (torch.float32, torch.bfloat16):
        if dec.dim() == 4 and dec.shape[3] == 1:
            dec = dec[..., 0]
        if dec.dim() != 3 or tuple(dec.shape) != (B, 2, N):
            raise ValueError('logits must be [%d, 2, %d, 1] or [%d, 2, %d], got %s' % (B, N, B, N, tuple(dec.shape)))
        kind = _hip.PGM_DEC_F32 if dec.dtype == torch.float32 else _hip.PGM_DEC_BF16
        sb, cs, vs = dec.stride()
    elif dec.dtype == torch.int64:
        if tuple(dec.shape) != (B, N):
            raise ValueError('assignments must be [%d, %d], got %s' % (B, N, tuple(dec.shape)))
        kind = _hip.PGM_DEC_I64
        (sb, vs), cs = dec.stride(), 0
    else:
        raise ValueError('decisions must be f32 / bf16 logits or int64 assignments, got %s' % dec.dtype)
    if not dec.is_cuda:
        raise RuntimeError('score runs on a ROCm device (no CPU fallback)')
    dev = dec.device
    logits = kind != _hip.PGM_DEC_I64
    if out is None:
        out = {'correct': torch.empty(B, dtype=torch.int32, device=dev), 'feasible': torch.empty(B, dtype=torch.uint8, device=dev),
               'objective': torch.empty(B, dtype=torch.float64, device=dev)}
        if logits:
            out['nll'] = torch.empty(B, dtype=torch.float64, device=dev)
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (4,) or counts.device != dev):
        raise ValueError('counts must be a [4] int64 tensor on %s' % dev)
    if B > 0:
        label = label.to(dev)
        if label.stride(1) != 1:
            label = label.contiguous()
        u = unary.to(dev, torch.float32).contiguous()
        p = pair.to(dev, torch.float32).contiguous()
        c = caps.to(dev, torch.int32).contiguous()
        bs = lambda t: 0 if t.shape[0] == 1 and B != 1 else t[0].numel()
        _hip.call('fgnn_chain_budget_score', dec, kind, sb, cs, vs, label, label.stride(0), u, u[0].numel(), p, bs(p), c, bs(c), B, N,
                  int(h), out.get('correct'), out.get('feasible'), out.get('objective'), out.get('nll') if logits else None, counts)
    res = dict(out)
    res['feasible'] = res['feasible'].view(torch.bool)
    return res


def _read_items(path, size):
    items = []
    with open(path, 'rb') as f:
        while size is None or len(items) < size:
            try:
                items.append(pickle.load(f))
            except EOFError:
                break
    if size is not None and len(items) < size:
        raise ValueError('%s holds %d items, %d asked for' % (path, len(items), size))
    return items


def load_test_set(path, family, size=None, device='cuda'):
    """The first ``size`` items (all when None) of a test set in the reference's pickle stream (one ``pickle.dump`` per item, as
    data_generate/generate_random_pgm.py and ``PgmDataPath.write_reference_dataset`` write it; ``RandomPGMData``'s item formats:
    raw (node_feature, assign, assign1), pws (node_feature, pws, assign, assign1), hops (node_feature, pws, hop, assign, assign1)).

    Returns device tensors in ``PgmDataPath.sample``'s tuple order, then the LP-relaxation label: hops (node_feature [n, 2, N, 1],
    pws [n, 4, N, 1], hops [n, h, N, 1], label, lp), pws (node_feature, pws, label, lp), raw (node_feature, label, lp); features
    f32, labels [n, N] int64; lp is None when every ``assign1`` is -1 (a file written without it).  The potentials are not in the
    items' features alone: raw items carry no link table or cap (``evaluate`` takes the generator's ``transition`` and ``cap``),
    pws items no cap; hops items carry theirs as the hop feature's one-hot."""
    _check_family(family)
    items = _read_items(path, None if size is None else int(size))
    nf = {'raw': 3, 'pws': 4, 'hops': 5}[family]
    if not items:
        raise ValueError('%s holds no items' % path)
    if any(len(it) != nf for it in items):
        raise ValueError('%s: %s items have %d fields' % (path, family, nf))
    cols = [np.stack([np.asarray(it[k]) for it in items]) for k in range(nf)]
    n, node = len(items), cols[0].astype(np.float32)
    if node.ndim == 3:
        node = node[..., None]
    N = node.shape[2]
    if node.shape[1:] != (2, N, 1):
        raise ValueError('node_feature must be [2, N] or [2, N, 1], got %s' % (node.shape[1:],))
    feats = [node]
    if family != 'raw':
        feats.append(cols[1].astype(np.float32).reshape(n, 4, N, 1))
    if family == 'hops':
        feats.append(cols[2].astype(np.float32).reshape(n, -1, N, 1))
    label, lp = cols[-2].astype(np.int64).reshape(n, N), cols[-1].astype(np.int64).reshape(n, N)
    dev = torch.device(device)
    out = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in feats + [label])
    return out + (None if (lp == -1).all() else torch.from_numpy(lp).to(dev),)


def make_test_set(path, family, size, seed=0, device='cuda', cap=CAP, transition=TRANSITION, hop_order=HOP_ORDER, chain_length=30):
    """Write a test set of ``size`` items with both labels (``write_reference_dataset(..., lp_label=True)``), drawn from (seed, steps
    TEST_STEP, TEST_STEP + 1, ...): the Philox counters of a training loop that passes its iteration as the step (from 0) never
    reach them, so a test set shares no item with training batches of any seed below 2^62 steps."""
    _check_family(family)
    PgmDataPath(device, chain_length, hop_order).write_reference_dataset(path, family, int(size), int(seed), step=TEST_STEP,
                                                                         cap=cap, transition=transition, lp_label=True)


def _edge_mlp(cin):
    C = torch.nn.Conv2d
    return torch.nn.Sequential(C(cin, 64, 1), torch.nn.ReLU(inplace=True), C(64, 16, 1))


def build_model(family, model_name=None):
    """(model, edge models) as the family's script builds them with its argparse defaults, on the CPU in training mode:
    raw (train_syn_fixed_pw_hop.py:118-172, default 'mp_nn'; 'mp_nn_comp', 'simple_gnn', 'iid') -> (mp_sequential, (emodel,));
    pws (train_syn_pw_factor.py:172-183) and hops (train_syn_hop_factor.py:172-183), 'mp_nn_factor' ->
    (factor_mpnn(2, [4, 1 or 9], ...), (emodel_pw, emodel_high))."""
    _check_family(family)
    from . import factor_mpnn, mp_conv_residual as R, mp_conv_type, mp_conv_v2, mp_sequential
    name = model_name or MODEL_NAMES[family][0]
    if name not in MODEL_NAMES[family]:
        raise ValueError('model_name for %s must be one of %s, got %r' % (family, MODEL_NAMES[family], name))
    C, BN, ReLU = torch.nn.Conv2d, torch.nn.BatchNorm2d, lambda: torch.nn.ReLU(inplace=True)
    with contextlib.redirect_stdout(sys.stderr):               # (the modules' constructors talk)
        if family != 'raw':
            model = factor_mpnn(2, [4, 1 if family == 'pws' else HOP_ORDER], [64, 64, 128, 128, 256, 256, 128, 128, 64, 64, 2],
                                [16, 16])
            return model, (_edge_mlp(3), _edge_mlp(1 if family == 'pws' else 2))
        head = mp_conv_v2(2, 64, 16, extension=mp_conv_type.ORIG_WITH_NEIGHBOR)
        if name == 'iid':
            model = mp_sequential(C(2, 64, 1), torch.nn.ReLU(True), C(64, 2, 1))
        elif name == 'simple_gnn':
            model = mp_sequential(head, R(64, 64, 16), C(64, 2, 1))
        else:
            mid = [R(256, 64, 16) for _ in range(1 if name == 'mp_nn' else 5)]
            model = mp_sequential(head, R(64, 64, 16), C(64, 128, 1), BN(128), ReLU(), R(128, 64, 16), C(128, 256, 1), BN(256),
                                  ReLU(), *mid, C(256, 128, 1), BN(128), ReLU(), R(128, 64, 16), C(128, 64, 1), BN(64), ReLU(),
                                  R(64, 64, 16), C(64, 2, 1))
        return model, (_edge_mlp(1),)


def load_checkpoint(path, family, model_name=None, device=None):
    """``build_model`` loaded from a checkpoint in the scripts' format (a dict with 'model_state_dict' and 'emodel_state_dict'
    (raw) or 'emodel_pw_state_dict' and 'emodel_high_state_dict' (pws, hops); the optimizer entries beside them are ignored), read
    with ``torch.load(weights_only=True)`` and loaded strictly.  A missing entry raises KeyError."""
    model, edge = build_model(family, model_name)
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    keys = ('model_state_dict',) + EDGE_KEYS[family]
    missing = [k for k in keys if k not in ckpt]
    if missing:
        raise KeyError('%s: no %s in the checkpoint (keys: %s)' % (path, ', '.join(missing), sorted(ckpt)))
    model.load_state_dict(ckpt['model_state_dict'], strict=True)
    for m, k in zip(edge, EDGE_KEYS[family]):
        m.load_state_dict(ckpt[k], strict=True)
    if device is not None:
        model.to(device)
        for m in edge:
            m.to(device)
    return model, edge


_TABLES = {}


def _tables(family, N, h, dev):
    """The family's static graph tables on ``dev`` with a leading batch axis of 1 (the scripts' generate_*_table outputs)."""
    key = (family, N, h, str(dev))
    if key not in _TABLES:
        from . import tables
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)[None]
        if family == 'raw':
            idx, ef = tables.knn_table(N, 8)                     # --neighbour 8
            _TABLES[key] = (t(idx), t(ef))
        else:
            pw_idx, pw_ef = tables.pw_factor_table(N)
            if family == 'pws':
                hi_idx, hi_ef, hi_feat = tables.chain_high_table(N, 9)       # --neighbour 9
                _TABLES[key] = (t(pw_idx), t(pw_ef), t(hi_idx), t(hi_ef), t(hi_feat))
            else:
                hi_idx, hi_ef = tables.ring_hop_table(N, h)
                _TABLES[key] = (t(pw_idx), t(pw_ef), t(hi_idx), t(hi_ef))
    return _TABLES[key]


def run_batch(model, edge_models, family, feats, hop_order=HOP_ORDER):
    """The model's output [B, 2, N, 1] on one batch of inputs (``feats``: node_feature [, pws [, hops]]), called as the family's
    test loop calls it (train_syn_fixed_pw_hop.py:331-334, train_syn_pw_factor.py:370-379, train_syn_hop_factor.py:368-377): the
    edge types from the edge models on the static edge features, the tables for every sample (``expand`` instead of the scripts'
    ``repeat``: the same values, no copies); pws's high-order factor feature is the zero [1, 1, 1] one.  No mode or grad change."""
    nf = feats[0]
    if nf.dim() == 3:
        nf = nf.unsqueeze(-1)
    B, N, dev = nf.shape[0], nf.shape[2], nf.device
    tabs = _tables(family, N, hop_order, dev)
    if family == 'raw':
        idx, ef = tabs
        et = edge_models[0](ef)
        return model(nf, idx.expand(B, -1, -1), et.expand(B, -1, -1, -1))
    pw_idx, pw_ef, hi_idx, hi_ef = tabs[:4]
    et_pw, et_hi = edge_models[0](pw_ef), edge_models[1](hi_ef)
    high = tabs[4].expand(B, -1, -1, -1) if family == 'pws' else feats[2]
    pred, _ = model(nf, [feats[1], high], [[pw_idx.expand(B, -1, -1), et_pw.expand(B, -1, -1, -1)],
                                           [hi_idx.expand(B, -1, -1), et_hi.expand(B, -1, -1, -1)]])
    return pred


def loop_figures(correct, nll, lp_correct, N, batch_size):
    """The reference test loop's figures from per-sample counts in file order, batches of ``batch_size`` (the last may be short):
    acc = accum_acc / gcnt, the mean of the per-batch accuracies ``all_correct.item() / np.prod(nlabel.shape)``; stddev =
    ``statistics.stdev`` of them (NaN below two batches, where the reference raises); loss = the mean of the per-batch mean NLLs
    (the per-batch ``F.cross_entropy``); the same for the LP label (None without it).  ``pooled`` is right / compared overall."""
    correct = np.asarray(correct, np.int64)
    n = len(correct)
    accs, accs_lp, losses = [], [], []
    for s in range(0, n, batch_size):
        e = min(n, s + batch_size)
        tot = (e - s) * N
        accs.append(int(correct[s:e].sum()) / tot)
        if lp_correct is not None:
            accs_lp.append(int(np.asarray(lp_correct[s:e], np.int64).sum()) / tot)
        if nll is not None:
            losses.append(float(np.sum(nll[s:e])) / tot)
    sd = lambda a: statistics.stdev(a) if len(a) >= 2 else float('nan')
    acc_sum = 0
    for a in accs:
        acc_sum += a
    out = {'acc': acc_sum / len(accs), 'stddev': sd(accs), 'loss': float(np.mean(losses)) if losses else None,
           'pooled_acc': int(correct.sum()) / (n * N), 'batches': len(accs)}
    if lp_correct is None:
        out.update(acc_lp=None, stddev_lp=None, pooled_acc_lp=None)
    else:
        lp_sum = 0
        for a in accs_lp:
            lp_sum += a
        out.update(acc_lp=lp_sum / len(accs_lp), stddev_lp=sd(accs_lp),
                   pooled_acc_lp=int(np.asarray(lp_correct, np.int64).sum()) / (n * N))
    return out


def map_figures(correct, feasible, objective, map_objective, N):
    """MAP-quality figures of n decisions: feasible fraction, exact-MAP fraction (every variable equal to the label), optimal
    fraction (feasible, objective within OPT_RTOL relative of the MAP's) and the mean relative gap (obj_MAP - obj) / |obj_MAP| over
    the feasible decisions (NaN when none is)."""
    correct, feasible = np.asarray(correct), np.asarray(feasible, bool)
    objective, map_objective = np.asarray(objective, np.float64), np.asarray(map_objective, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = (map_objective - objective) / np.abs(map_objective)
    optimal = feasible & (np.abs(map_objective - objective) <= OPT_RTOL * np.abs(map_objective))
    return {'feasible': float(feasible.mean()), 'exact_map': float((correct == N).mean()), 'optimal': float(optimal.mean()),
            'mean_gap': float(gap[feasible].mean()) if feasible.any() else float('nan')}


def evaluate(model, edge_models, test_set, family, batch_size=32, eval_batch=4096, cap=CAP, transition=TRANSITION,
             hop_order=HOP_ORDER, return_logits=False, bp=False, bp_args=None):
    """The family's test loop on ``test_set`` (``load_test_set``'s tuple, or a path to read with it) and the MAP-quality figures.

    The model and edge models run in eval mode under no_grad (their training flags are restored afterwards) in chunks of
    ``eval_batch`` items; ``score`` counts each chunk on the device, and the host reads the per-sample results back once, at the
    end.  In eval mode an item's logits depend on the chunk it is in only through rounding (BatchNorm uses its running statistics,
    InstanceNorm is per sample, but another batch size can dispatch another kernel), so a decision within rounding of a tie may
    flip between ``eval_batch`` values.  The reference's figures are then formed from the per-sample counts over consecutive
    batches of ``batch_size`` in file order (``loop_figures``).  The reference's pws / hops test loaders shuffle, so its stddev is a
    random quantity; this one is the file-order one.

    ``test_set``: ``load_test_set``'s tuple (or ``sample(..., lp_label=True)``'s); the potentials are rebuilt from it as
    ``PgmDataPath.lp_inputs`` does, with ``cap`` and ``transition`` where the items do not carry them.

    Returns a dict: acc, acc_lp, stddev, stddev_lp, loss, pooled_acc, pooled_acc_lp (acc_lp etc. None when the file has no LP
    label), 'model' and 'lp' (``map_figures``: feasible, exact_map, optimal, mean_gap; 'lp' None without the label), 'map_feasible'
    (the labels' own feasible fraction: 1 for exact labels), n, N; with return_logits also 'logits' [n, 2, N, 1] on the device.

    With ``bp`` the max-product baseline is solved per chunk on the same potentials (``PgmDataPath.solve_bp(**bp_args)``; stored test
    sets carry no such label) and scored by the same kernel: acc_bp, stddev_bp, pooled_acc_bp (``loop_figures``' arithmetic), 'bp'
    (``map_figures``) and bp_converged, the fraction of samples that stopped below the tolerance (status 0).  Without it the
    dict has none of these keys."""
    _check_family(family)
    if isinstance(test_set, (str, os.PathLike)):
        test_set = load_test_set(test_set, family, device=next(model.parameters()).device)
    batch_size, eval_batch = int(batch_size), int(eval_batch)
    if batch_size < 1 or eval_batch < 1:
        raise ValueError('batch_size and eval_batch must be >= 1')
    bp_args = dict(bp_args or {})
    if set(bp_args) - {'max_iter', 'damping', 'tol'}:
        raise ValueError('bp_args takes max_iter, damping and tol, got %s' % sorted(bp_args))
    *feats, label, lp = test_set
    n, N = label.shape
    dev = label.device
    h = feats[2].shape[1] if family == 'hops' else int(hop_order)
    path = PgmDataPath(dev, N, h)
    if bp:
        check_bp_args(N, h, **bp_args)
    unary, pair, caps = path.lp_inputs(family, tuple(feats) + (label,), cap, transition)
    if not torch.is_tensor(caps):                                  # (once on the device: no host copy per chunk)
        caps = torch.full((N - h + 1,), int(caps), dtype=torch.int32, device=dev)
    cut = lambda s, e: (unary[s:e], pair[s:e] if pair.dim() == 3 else pair, caps[s:e] if caps.dim() == 2 else caps)

    def outs(logits):
        o = {'correct': torch.empty(n, dtype=torch.int32, device=dev), 'feasible': torch.empty(n, dtype=torch.uint8, device=dev),
             'objective': torch.empty(n, dtype=torch.float64, device=dev)}
        if logits:
            o['nll'] = torch.empty(n, dtype=torch.float64, device=dev)
        return o

    res_m, res_map = outs(True), outs(False)
    res_lp = outs(False) if lp is not None else None
    res_bp = outs(False) if bp else None
    bp_status = torch.empty(n, dtype=torch.int32, device=dev) if bp else None
    logits_all = torch.empty((n, 2, N, 1), dtype=torch.float32, device=dev) if return_logits else None
    mods = [model] + list(edge_models)
    was = [m.training for m in mods]
    for m in mods:
        m.eval()
    try:
        with torch.no_grad():
            for s in range(0, n, eval_batch):
                e = min(n, s + eval_batch)
                pred = run_batch(model, edge_models, family, [f[s:e] for f in feats], h)
                if return_logits:
                    logits_all[s:e] = pred
                u, p, c = cut(s, e)
                sl = lambda o: {k: v[s:e] for k, v in o.items()}
                score(pred, label[s:e], u, p, c, h, out=sl(res_m))
                score(label[s:e], label[s:e], u, p, c, h, out=sl(res_map))
                if lp is not None:
                    score(lp[s:e], label[s:e], u, p, c, h, out=sl(res_lp))
                if bp:
                    bp_label, det = path.solve_bp(u, p, c, want_details=True, **bp_args)
                    bp_status[s:e] = det['status']
                    score(bp_label, label[s:e], u, p, c, h, out=sl(res_bp))
    finally:
        for m, w in zip(mods, was):
            m.train(w)
    keys = ('correct', 'feasible', 'objective')
    cols = [res_m[k].double() for k in keys + ('nll',)] + [res_map[k].double() for k in keys]
    if lp is not None:
        cols += [res_lp[k].double() for k in keys]
    if bp:
        cols += [res_bp[k].double() for k in keys] + [bp_status.double()]
    host = torch.stack(cols).cpu().numpy()                          # the one read-back
    mc, mf, mo, mn, _, pf, po = host[:7]
    out = loop_figures(mc.astype(np.int64), mn, host[7].astype(np.int64) if lp is not None else None, N, batch_size)
    out['model'] = map_figures(mc, mf > 0, mo, po, N)
    out['lp'] = map_figures(host[7], host[8] > 0, host[9], po, N) if lp is not None else None
    out['map_feasible'] = float((pf > 0).mean())
    if bp:
        bc, bf, bo, bs = host[-4:]
        fig = loop_figures(mc.astype(np.int64), None, bc.astype(np.int64), N, batch_size)      # (the LP slot's arithmetic)
        out.update(acc_bp=fig['acc_lp'], stddev_bp=fig['stddev_lp'], pooled_acc_bp=fig['pooled_acc_lp'],
                   bp=map_figures(bc, bf > 0, bo, po, N), bp_converged=float((bs == 0).mean()))
    out['n'], out['N'] = int(n), int(N)
    if return_logits:
        out['logits'] = logits_all
    return out


def _fmt(x):
    return 'n/a' if x is None else '%.6f' % x


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m fgnn_amd.pgm_eval',
                                 description="Evaluate a synthetic-PGM model on a stored test set (train_syn_*.py's test loop, plus "
                                             "feasibility and optimality of its decisions) or write a test set.")
    ap.add_argument('--family', choices=sorted(FAMILIES), default='hops')
    ap.add_argument('--test_path', help="test set in the reference's pickle stream")
    ap.add_argument('--test_size', type=int, default=None, help='items to read (default: all)')
    ap.add_argument('--model_path', help="checkpoint in the family script's format")
    ap.add_argument('--model_name', default=None, help='raw: mp_nn (default), mp_nn_comp, simple_gnn, iid; pws / hops: mp_nn_factor')
    ap.add_argument('--batch_size', type=int, default=32, help="the reference loop's batch (its figures' grouping)")
    ap.add_argument('--eval_batch', type=int, default=4096, help='items per model call')
    ap.add_argument('--transition', type=float, nargs=4, default=list(TRANSITION), help='raw: the link table')
    ap.add_argument('--cap', type=int, default=CAP, help='raw / pws: the budget')
    ap.add_argument('--bp', action='store_true', help='also solve and score the max-product belief-propagation baseline')
    ap.add_argument('--json', action='store_true', help='print the figures as one JSON line instead')
    ap.add_argument('--make_test_set', metavar='PATH', help='write a test set with both labels to PATH and stop')
    ap.add_argument('--num', type=int, default=10000, help='items (--make_test_set)')
    ap.add_argument('--seed', type=int, default=0, help='--make_test_set')
    args = ap.parse_args(argv)
    dev = torch.device('cuda:0')
    if args.make_test_set:
        make_test_set(args.make_test_set, args.family, args.num, args.seed, dev, cap=args.cap, transition=args.transition)
        return 0
    if not args.test_path or not args.model_path:
        ap.error('give --test_path and --model_path, or --make_test_set')
    model, edge = load_checkpoint(args.model_path, args.family, args.model_name, dev)
    ts = load_test_set(args.test_path, args.family, args.test_size, dev)
    r = evaluate(model, edge, ts, args.family, args.batch_size, args.eval_batch, cap=args.cap, transition=args.transition,
                 bp=args.bp)
    if args.json:
        clean = lambda v: {k: clean(x) for k, x in v.items()} if isinstance(v, dict) else (None if isinstance(v, float) and
                                                                                         math.isnan(v) else v)
        print(json.dumps(clean(r)))
        return 0
    print('testing result: acc = {}, acc_lp = {}'.format(r['acc'], r['acc_lp']))
    print('stddev = {}, stddev_lp = {}'.format(r['stddev'], r['stddev_lp']))
    print('loss = {}, pooled acc = {}, pooled acc_lp = {}'.format(r['loss'], r['pooled_acc'], r['pooled_acc_lp']))
    if args.bp:
        print('acc_bp = {}, stddev_bp = {}, pooled acc_bp = {}, bp converged = {}'.format(r['acc_bp'], r['stddev_bp'],
                                                                                          r['pooled_acc_bp'], r['bp_converged']))
    for who in ('model', 'lp') + (('bp',) if args.bp else ()):
        f = r[who]
        if f is None:
            print('%-5s  (no LP label in the test set)' % who)
            continue
        print('%-5s  feasible %s  exact MAP %s  optimal %s  mean gap %s' % (who, _fmt(f['feasible']), _fmt(f['exact_map']),
                                                                          _fmt(f['optimal']), _fmt(f['mean_gap'])))
    return 0


if __name__ == '__main__':
    sys.exit(main())
