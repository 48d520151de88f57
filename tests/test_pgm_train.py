"""Host side of the synthetic-PGM trainer (fgnn_amd/pgm_train.py): the new C entry points' presence and argument checks, the CPU
form of the clipped FlatAdam, the schedule arithmetic, the checkpoint layout and labelling_loss's input checks.  No GPU needed."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('fgnn_pgm_loss_forward', 'fgnn_pgm_loss_backward', 'fgnn_pgm_loss_workspace_bytes', 'fgnn_grad_norm_clip',
       'fgnn_grad_norm_clip_workspace_bytes', 'fgnn_flat_adam_clipped', 'fgnn_flat_adam_dev_clipped')
EINVAL = -1


def test_new_entry_points_are_exported_declared_and_built():
    from fgnn_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'fgnn_hip.h')).read()
    L = _hip.lib()
    for name in NEW:
        assert name in _hip.EXPORTS
        assert re.search(r'\b%s\(' % name, header), name
        fn = getattr(L, name)
        assert fn.argtypes is not None
    assert _hip.ABI_VERSION == 15 and L.fgnn_abi_version() == 15
    assert '#define FGNN_ABI_VERSION 15' in header
    later = header[header.index('later additions at 15'):header.index('#define FGNN_ABI_VERSION')]
    assert all(name in later for name in NEW)


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    """Every check runs before any launch: 1 <= N <= 1024 else FGNN_EUNSUPPORTED; null pointers, negative sizes or strides and a
    short workspace FGNN_EINVAL."""
    from fgnn_amd import _hip
    L = _hip.lib()
    p = ctypes.c_void_p(4096)                      # non-NULL, 16-byte aligned, never dereferenced on these paths
    ws = int(L.fgnn_pgm_loss_workspace_bytes())
    assert ws >= 8 and ws % 8 == 0

    def fwd(logits=p, kind=_hip.PGM_DEC_F32, sb=60, cs=30, vs=1, label=p, lsb=30, lp=None, lpsb=0, B=4, N=30, loss=p, counts=None,
            w=p, wb=ws):
        return L.fgnn_pgm_loss_forward(logits, kind, sb, cs, vs, label, lsb, lp, lpsb, B, N, loss, counts, w, wb, None)

    assert fwd(logits=None) == EINVAL and b'null' in L.fgnn_last_error()
    assert fwd(label=None) == EINVAL and fwd(loss=None) == EINVAL and fwd(w=None) == EINVAL
    assert fwd(N=0) == _hip.EUNSUPPORTED and fwd(N=1025) == _hip.EUNSUPPORTED and b'1025' in L.fgnn_last_error()
    assert fwd(kind=_hip.PGM_DEC_I64) == _hip.EUNSUPPORTED
    assert fwd(sb=-1) == EINVAL and fwd(cs=-1) == EINVAL and fwd(vs=-1) == EINVAL and fwd(lsb=-1) == EINVAL and fwd(lpsb=-1) == EINVAL
    assert fwd(B=-1) == EINVAL and fwd(N=-1) == EINVAL
    assert fwd(wb=ws - 8) == EINVAL and b'workspace' in L.fgnn_last_error()

    def bwd(logits=p, kind=_hip.PGM_DEC_BF16, sb=60, cs=30, vs=1, label=p, lsb=30, gloss=p, B=4, N=30, g=p, gsb=60, gcs=30, gvs=1):
        return L.fgnn_pgm_loss_backward(logits, kind, sb, cs, vs, label, lsb, gloss, B, N, g, gsb, gcs, gvs, None)

    assert bwd(logits=None) == EINVAL and bwd(label=None) == EINVAL and bwd(gloss=None) == EINVAL and bwd(g=None) == EINVAL
    assert bwd(N=0) == _hip.EUNSUPPORTED and bwd(N=1025) == _hip.EUNSUPPORTED
    assert bwd(sb=-1) == EINVAL and bwd(gsb=-1) == EINVAL and bwd(gcs=-1) == EINVAL and bwd(gvs=-1) == EINVAL and bwd(B=-1) == EINVAL
    assert bwd(B=0) == 0                           # an empty batch: nothing to write

    nws = int(L.fgnn_grad_norm_clip_workspace_bytes())
    assert nws >= 8 and nws % 8 == 0
    norm = lambda g=p, n=64, out=p, w=p, wb=nws: L.fgnn_grad_norm_clip(g, n, 1.0, 1.0, out, w, wb, None)
    assert norm(g=None) == EINVAL and norm(out=None) == EINVAL and norm(w=None) == EINVAL
    assert norm(n=-1) == EINVAL and norm(wb=nws - 8) == EINVAL and b'workspace' in L.fgnn_last_error()
    assert norm(g=ctypes.c_void_p(4100)) == EINVAL

    adam = lambda param=p, clip=p, n=64, step=1: L.fgnn_flat_adam_clipped(param, p, p, p, None, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0,
                                                                           step, clip, None)
    assert adam(clip=None) == EINVAL and b'clip' in L.fgnn_last_error()
    assert adam(param=None) == EINVAL and adam(n=-1) == EINVAL and adam(step=0) == EINVAL
    assert adam(n=0) == 0
    dev = lambda param=p, clip=p, lr=p, n=64: L.fgnn_flat_adam_dev_clipped(param, p, p, p, None, n, lr, 0.9, 0.999, 1e-8, 0.0, 1.0, p, p,
                                                                           clip, None)
    assert dev(clip=None) == EINVAL and dev(param=None) == EINVAL and dev(lr=None) == EINVAL and dev(n=-1) == EINVAL


@pytest.mark.parametrize('scale', [40.0, 0.01], ids=['clipped', 'not_clipped'])
def test_cpu_flat_adam_with_max_grad_norm_matches_clip_grad_norm_and_torch_adam(scale):
    """dp.FlatAdam(max_grad_norm=1.0) on the CPU == torch.nn.utils.clip_grad_norm_(params, 1.0) + torch.optim.Adam over the
    separate tensors (odd sizes), 5 steps, with gradients whose norm is above 1 (clipped) and below (coefficient 1).  Tolerance: that
    of the unclipped comparison, tests/test_host_logic.py:247 (rtol 1e-5, atol 1e-7)."""
    from fgnn_amd.dp import FlatAdam, FlatGradBucket

    def make():
        torch.manual_seed(3)
        return [torch.nn.Parameter(torch.randn(s)) for s in ((7, 5), (3,), (1,), (11, 3), (13,))]

    a, b = make(), make()
    ref = torch.optim.Adam(a, lr=1e-2, weight_decay=1e-3)
    bucket = FlatGradBucket(b, flatten_params=True)
    opt = FlatAdam(bucket, lr=1e-2, weight_decay=1e-3, max_grad_norm=1.0)
    g = torch.Generator().manual_seed(5)
    for _ in range(5):
        grads = [torch.randn(q.shape, generator=g) * scale for q in a]
        ref.zero_grad()
        bucket.zero()
        for qa, qb, gr in zip(a, b, grads):
            qa.grad = gr.clone()
            qb.grad.copy_(gr)
        total = torch.nn.utils.clip_grad_norm_(a, 1.0)
        ref.step()
        opt.step()
        assert (float(total) > 1.0) == (scale > 1.0)
        assert torch.allclose(opt.grad_norm, total.reshape(1), rtol=1e-6, atol=0)
        assert opt.grad_norm.shape == (1,)
    for qa, qb in zip(a, b):
        assert torch.allclose(qa, qb, rtol=1e-5, atol=1e-7), float((qa - qb).abs().max())


def test_fast_adam_passes_max_grad_norm_through_and_keeps_the_stock_layout():
    from fgnn_amd.fastpath import FastAdam
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(3))]
    opt = FastAdam(ps, lr=1e-2, max_grad_norm=1.0)
    assert opt.flat.max_grad_norm == 1.0 and FastAdam([torch.nn.Parameter(torch.zeros(2))]).grad_norm is None
    for q in ps:
        q.grad.fill_(3.0)
    opt.step()
    assert abs(float(opt.grad_norm) - 3.0 * math.sqrt(18)) < 1e-4
    sd = opt.state_dict()
    assert 'max_grad_norm' not in sd['param_groups'][0]
    stock = torch.optim.Adam([torch.nn.Parameter(q.detach().clone()) for q in ps], lr=1e-2)
    stock.load_state_dict(sd)                      # a stock Adam resumes from it and steps
    for q in stock.param_groups[0]['params']:
        q.grad = torch.ones_like(q)
    stock.step()
    assert int(stock.state[stock.param_groups[0]['params'][0]]['step']) == 2


def test_schedule_matches_lambda_lr_driven_as_the_script_drives_it():
    """train_syn_*.py: scheduler.step() at the top of every epoch, before its batches.  Epoch e trains at 3e-3 max(0.98^(e+1), 1e-6)."""
    from fgnn_amd import pgm_train as T
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=3e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: max(0.98 ** x, 1e-6))
    import warnings
    for e in range(6):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sched.step()
        assert opt.param_groups[0]['lr'] == T.epoch_lr(e) == 3e-3 * max(0.98 ** (e + 1), 1e-6)
        opt.step()
    assert T.lr_lambda(10 ** 4) == 1e-6
    assert T.default_steps_per_epoch(32) == math.ceil(90000 / 32) == 2813
    assert T.default_steps_per_epoch(512) == 176 and T.default_steps_per_epoch(90000) == 1 and T.default_steps_per_epoch(90001) == 1
    with pytest.raises(ValueError):
        T.default_steps_per_epoch(0)


@pytest.mark.parametrize('family', ['raw', 'pws', 'hops'])
def test_checkpoint_dict_has_the_scripts_keys(family, tmp_path):
    """The family's get_model_dict keys; the dict survives torch.save / load(weights_only=True) and loads strictly into a fresh
    model (pgm_eval.load_checkpoint's way)."""
    from fgnn_amd import pgm_eval, pgm_train as T
    edge_keys = {'raw': ('emodel_state_dict',), 'pws': ('emodel_pw_state_dict', 'emodel_high_state_dict'),
                 'hops': ('emodel_pw_state_dict', 'emodel_high_state_dict')}[family]
    torch.manual_seed(1)
    model, edge = pgm_eval.build_model(family)
    opt = torch.optim.Adam([q for m in [model] + list(edge) for q in m.parameters()], lr=T.LR)
    sched = T._scheduler(opt)
    d = T.checkpoint_dict(family, model, edge, opt, sched, 3, 77)
    assert set(d) == {'model_state_dict', 'optimizer_state_dict', 'lr_sche', 'epoch', 'gcnt'} | set(edge_keys)
    assert d['epoch'] == 3 and d['gcnt'] == 77
    path = str(tmp_path / 'c.pt')
    torch.save(d, path)
    m2, e2 = pgm_eval.load_checkpoint(path, family)
    for k, v in model.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k])
    back = torch.load(path, map_location='cpu', weights_only=True)
    sched2 = T._scheduler(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=T.LR))
    sched2.load_state_dict(back['lr_sche'])
    assert sched2.last_epoch == sched.last_epoch
    assert T.checkpoint_path('out', family, 'm', 4) == os.path.join('out', 'm_%s_epoches_4.pt' % family)


def test_labelling_loss_rejects_bad_inputs_before_the_device():
    from fgnn_amd.pgm_train import labelling_loss
    pred, label = torch.zeros(4, 2, 30, 1), torch.zeros(4, 30, dtype=torch.int64)
    bad = [(pred, label.int()), (pred, label[0]), (pred.double(), label), (pred.half(), label), (torch.zeros(4, 3, 30, 1), label),
           (torch.zeros(4, 2, 31, 1), label), (torch.zeros(4, 2, 30, 2), label), (torch.zeros(5, 2, 30), label),
           (torch.zeros(1, 2, 1025), torch.zeros(1, 1025, dtype=torch.int64)), (torch.zeros(2, 2, 0), torch.zeros(2, 0, dtype=torch.int64))]
    for p, l in bad:
        with pytest.raises(ValueError):
            labelling_loss(p, l)
    with pytest.raises(ValueError):
        labelling_loss(pred, label, lp_label=label[:, :29])
    with pytest.raises(ValueError):
        labelling_loss(pred, label, lp_label=label.int())
    with pytest.raises(ValueError):
        labelling_loss(pred, label, counts=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        labelling_loss(pred, label, counts=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError):              # well-formed, but not on a ROCm device: no CPU fallback
        labelling_loss(pred, label, counts=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        labelling_loss(pred[..., 0].bfloat16(), label)
