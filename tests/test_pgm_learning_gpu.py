"""GPU: config 5 (factor_mpnn on the hops family, train_syn_hop_factor.py) learns from PgmDataPath batches.

The reference loop (/root/reference/train_syn_hop_factor.py:275-304): edge models -> factor_mpnn -> cross entropy against the exact
MAP labels -> backward -> gradient-norm clip 1.0 -> Adam 3e-3, f32.  Here every step draws a fresh batch in the kernel
(``sample(B, 'hops', seed, step)``) instead of reading the AD3-labelled pickle.  After STEPS steps the per-variable accuracy on a
held-out batch (eval mode) must beat the "argmax of the unary potentials" baseline on the same batch by MARGIN, and the loss must
have gone down.

First run on the MI355X (STEPS = 400, B = 512, held-out 4096 chains of another seed): 12.8 s of training, smoothed loss
0.602 -> 0.214, held-out accuracy 0.909 against a unary-argmax baseline of 0.592 (a margin of 0.32).  MARGIN = 0.15 and a loss
at most 0.7 x its start leave about half of that as room."""
import contextlib
import io
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

SYN_DIMS = [64, 64, 128, 128, 256, 256, 128, 128, 64, 64, 2]          # train_syn_hop_factor.py:171
STEPS, B, N, H = 400, 512, 30, 9
MARGIN = 0.15


def _setup(dev):
    import fgnn_amd
    from fgnn_amd import tables
    torch.manual_seed(0)
    C = torch.nn.Conv2d
    with contextlib.redirect_stdout(io.StringIO()):
        model = fgnn_amd.factor_mpnn(2, [4, H], SYN_DIMS, [16, 16]).to(dev)
    em_pw = torch.nn.Sequential(C(3, 64, 1), torch.nn.ReLU(inplace=True), C(64, 16, 1)).to(dev)
    em_hi = torch.nn.Sequential(C(2, 64, 1), torch.nn.ReLU(inplace=True), C(64, 16, 1)).to(dev)
    pw_idx, pw_ef = tables.pw_factor_table(N)
    hi_idx, hi_ef = tables.ring_hop_table(N, H)
    t = lambda a: torch.from_numpy(a).to(dev)[None]
    return model, em_pw, em_hi, (t(pw_idx), t(pw_ef), t(hi_idx), t(hi_ef))


def _forward(model, em_pw, em_hi, tabs, nf, pws, hops):
    idx_pw, ef_pw, idx_hi, ef_hi = tabs
    b = nf.shape[0]
    et_pw, et_hi = em_pw(ef_pw), em_hi(ef_hi)
    pred, _ = model(nf, [pws, hops], [[idx_pw.expand(b, -1, -1), et_pw.expand(b, -1, -1, -1)],
                                      [idx_hi.expand(b, -1, -1), et_hi.expand(b, -1, -1, -1)]])
    return pred.squeeze(-1).permute(0, 2, 1).contiguous()                 # [b, N, 2]


def test_config5_learns_on_exact_labels(dev):
    from fgnn_amd import PgmDataPath
    path = PgmDataPath(dev, N, H)
    model, em_pw, em_hi, tabs = _setup(dev)
    params = list(model.parameters()) + list(em_pw.parameters()) + list(em_hi.parameters())
    opt = torch.optim.Adam(params, lr=3e-3)
    for m in (model, em_pw, em_hi):
        m.train()
    losses = torch.zeros(STEPS, device=dev)
    t0 = time.time()
    for it in range(STEPS):
        nf, pws, hops, label = path.sample(B, 'hops', seed=0, step=it)
        opt.zero_grad()
        pred = _forward(model, em_pw, em_hi, tabs, nf, pws, hops)
        loss = torch.nn.functional.cross_entropy(pred.view(-1, 2), label.view(-1))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        losses[it] = loss.detach()
    torch.cuda.synchronize()
    train_s = time.time() - t0
    losses = losses.cpu()
    first, last = float(losses[:20].mean()), float(losses[-20:].mean())

    nf, pws, hops, label = path.sample(4096, 'hops', seed=1, step=0)    # held out: another seed
    for m in (model, em_pw, em_hi):
        m.eval()
    with torch.no_grad():
        pred = _forward(model, em_pw, em_hi, tabs, nf, pws, hops)
    acc = float((pred.argmax(-1) == label).float().mean())
    baseline = float(((nf[:, 1, :, 0] > nf[:, 0, :, 0]).long() == label).float().mean())
    print('config 5 on exact labels: %d steps x %d in %.1f s; loss %.4f -> %.4f; held-out accuracy %.4f, unary-argmax baseline %.4f'
          % (STEPS, B, train_s, first, last, acc, baseline))
    assert torch.isfinite(losses).all()
    assert last < 0.7 * first
    assert acc > baseline + MARGIN, (acc, baseline)
