"""csrc/mpconv_bwd_hyper.hip::mpconv_bwd_fanin_kernel — the backward of a constant-etype call with ONE destination of degree k — at
the edges of its schedule: batches smaller than a workgroup's eight waves and ragged ones, every winner on one row, as many distinct
winner rows as channels, one node, the wide instances, f32, and the layouts that take element accesses instead of 16-byte ones.
Every case compares dx, dW and dbias with torch autograd through the forward's own routing (the recorded argmax picks the
neighbour, as in test_mpconv_gpu.py), to 2^-7 relative in bf16 and 2e-5 in f32, and asserts that the fan-in kernel ran."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu


def _run(dev, x, idx, et, W, bias, gz, layout='channels_last'):
    """x [B,nin,N,1], idx [B,1,k], et [B,1,1,k], gz [B,nou,1,1] on the CPU in the storage dtype; W, bias f32.
    -> (gx, gW, gb) of the kernel on the CPU, (gx, gW, gb) of the routed f32 reference, the argmax [B,nou] the forward recorded."""
    from fgnn_amd import _hip, ops
    B, nou = x.shape[0], W.shape[1]
    xd = x.to(dev)
    if layout == 'channels_last':
        xd = xd.contiguous(memory_format=torch.channels_last)
    elif layout == 'unaligned':          # channel-fastest rows that start one element past a 16-byte boundary
        flat = torch.empty(x.numel() + 8, dtype=x.dtype, device=dev)
        xd = flat[1:1 + x.numel()].view(B, x.shape[2], 1, x.shape[1]).permute(0, 3, 1, 2)
        xd.copy_(x.to(dev))
        assert xd.data_ptr() % 16 != 0 and xd.stride(1) == 1
    xd = xd.detach().requires_grad_(True)
    Wd, bd = W.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    idx_d, et_d = idx.to(dev), et.to(dev)
    _, am = ops.mpconv_forward_raw(xd.detach(), idx_d, et_d, W.to(dev), bias.to(dev), nou, 1, 0, _hip.AGG_MAX, want_argmax=True)
    z = ops.mpconv(xd, idx_d, et_d, Wd, bd, nou, 1, 0, _hip.AGG_MAX)
    z.backward(gz.to(dev))
    name = _hip.lib().fgnn_last_kernel().decode()
    assert name.startswith('mpconv_bwd_fanin_kernel'), name
    xr = x.float().detach().clone().requires_grad_(True)
    Wr, br = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    P = torch.einsum('bcn,co->bno', xr[..., 0], Wr)                                 # [B,N,nou]
    E = P[torch.arange(B)[:, None, None], idx] * et.float()[:, 0, :, :, None]       # [B,1,k,nou]
    sel = am.cpu().long()[..., 0].permute(0, 2, 1)[:, :, None, :]                   # [B,1,1,nou]
    zr = E.gather(2, sel)[:, :, 0, :].permute(0, 2, 1)[..., None] + br[None, :, None, None]
    zr.backward(gz.float())
    return (xd.grad.cpu(), Wd.grad.cpu(), bd.grad.cpu()), (xr.grad, Wr.grad, br.grad), am.cpu().long()[:, :, 0, 0]


def _compare(got, ref, dtype):
    tol = 2e-5 if dtype == torch.float32 else 2.0 ** -7
    gx, gW, gb = got
    rx, rW, rb = ref
    ex, eW, eb = H.rel_err(gx.float(), rx), H.rel_err(gW, rW), H.rel_err(gb, rb)
    print('rel err dx %.3e dW %.3e dbias %.3e (tol %.3e)' % (ex, eW, eb, tol))
    assert ex <= tol
    assert eW <= tol
    assert eb <= tol
    assert bool(((rx == 0) <= (gx.float() == 0)).all())          # rows nobody routed to are exact zeros


def _inputs(B, nin, nou, N, k, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, nin, N, 1, generator=g).to(dtype)
    idx = torch.randint(0, N, (B, 1, k), generator=g)
    et = (torch.rand(B, 1, 1, k, generator=g) + 0.5).to(dtype)
    W = torch.randn(nin, nou, generator=g) * 0.1
    bias = torch.randn(nou, generator=g)
    gz = torch.randn(B, nou, 1, 1, generator=g).to(dtype)
    return x, idx, et, W, bias, gz


@pytest.mark.parametrize('B', [1, 3, 17])
def test_batches_below_and_across_a_workgroup(B, dev):
    """Fewer samples than the eight waves of a workgroup (waves without a sample still take part in the fold) and a ragged batch."""
    x, idx, et, W, bias, gz = _inputs(B, 64, 64, 96, 96, torch.bfloat16, 100 + B)
    got, ref, _ = _run(dev, x, idx, et, W, bias, gz)
    _compare(got, ref, torch.bfloat16)


def test_all_winners_on_one_row(dev):
    """Every slot names node 37: all 64 channels' gradients land in that row, the other 95 rows are exact zeros."""
    B, N = 5, 96
    x, idx, et, W, bias, gz = _inputs(B, 64, 64, N, 96, torch.bfloat16, 7)
    idx = torch.full_like(idx, 37)
    got, ref, _ = _run(dev, x, idx, et, W, bias, gz)
    _compare(got, ref, torch.bfloat16)
    gx = got[0].float()[..., 0]                                   # [B,nin,N]
    others = torch.ones(N, dtype=torch.bool)
    others[37] = False
    assert bool((gx[:, :, others] == 0).all())
    assert bool((gx[:, :, 37] != 0).any())


@pytest.mark.parametrize('nou', [64, 128])
def test_as_many_distinct_winner_rows_as_channels(nou, dev):
    """N = k = 64, the identity table, W = I (or [I | I]) and x[b, c, n] = [c == n] + small noise: row n wins channel n (and n + 64),
    nothing else — 64 touched rows, the longest dx path."""
    B, nin, N = 5, 64, 64
    g = torch.Generator().manual_seed(21 + nou)
    x = (torch.eye(nin)[None, :, :, None] + 0.01 * torch.randn(B, nin, N, 1, generator=g)).to(torch.bfloat16)
    idx = torch.arange(N).reshape(1, 1, N).repeat(B, 1, 1)
    et = torch.ones(B, 1, 1, N, dtype=torch.bfloat16)
    W = torch.cat([torch.eye(nin)] * (nou // nin), dim=1).contiguous()
    bias = torch.randn(nou, generator=g)
    gz = torch.randn(B, nou, 1, 1, generator=g).to(torch.bfloat16)
    got, ref, am = _run(dev, x, idx, et, W, bias, gz)
    assert torch.equal(am, (torch.arange(nou) % nin)[None, :].expand(B, -1))     # the routing is what the case is about
    _compare(got, ref, torch.bfloat16)
    assert bool((ref[0][..., 0] != 0).any(dim=1).all())           # every row received something


def test_single_node(dev):
    x, idx, et, W, bias, gz = _inputs(9, 64, 64, 1, 1, torch.bfloat16, 3)
    got, ref, _ = _run(dev, x, idx, et, W, bias, gz)
    _compare(got, ref, torch.bfloat16)


@pytest.mark.parametrize('nin,nou', [(128, 64), (64, 128)])
def test_wide_instances(nin, nou, dev):
    x, idx, et, W, bias, gz = _inputs(17, nin, nou, 96, 96, torch.bfloat16, nin + 2 * nou)
    got, ref, _ = _run(dev, x, idx, et, W, bias, gz)
    _compare(got, ref, torch.bfloat16)


def test_f32_instance(dev):
    x, idx, et, W, bias, gz = _inputs(9, 64, 64, 96, 96, torch.float32, 5)
    got, ref, _ = _run(dev, x, idx, et, W, bias, gz)
    _compare(got, ref, torch.float32)


@pytest.mark.parametrize('layout', ['nchw', 'unaligned'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_layouts_without_16_byte_rows(layout, dtype, dev):
    """Node-fastest states and channel-fastest ones off a 16-byte boundary: no layout is turned down (the NCHW calls of
    test_mpconv_gpu.py must report this kernel), they run the same schedule with element accesses; the gradients are the
    same as the channel-fastest call's, bit for bit, whenever both forwards recorded the same winners."""
    x, idx, et, W, bias, gz = _inputs(11, 64, 64, 40, 40, dtype, 9)
    got, ref, am = _run(dev, x, idx, et, W, bias, gz, layout=layout)
    _compare(got, ref, dtype)
    packed, _, am_packed = _run(dev, x, idx, et, W, bias, gz)
    if torch.equal(am, am_packed):       # (another forward kernel may settle a near-tie differently)
        assert all(torch.equal(a, b) for a, b in zip(got, packed))
