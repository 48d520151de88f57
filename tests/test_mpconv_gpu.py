"""GPU parity of the fused HIP message operator (through the C ABI) against
(a) the golden vectors the real reference produced and (b) the CPU oracle on fresh seeded inputs.
Tolerance for fp32: 1e-4 (BASELINE.json north_star), tightened to 2e-5 relative where the math
is a single operator call."""
import contextlib
import pytest
import torch

import fgnn_oracle as O
import helpers as H

pytestmark = pytest.mark.gpu

CASES = H.operator_cases()
TOL = 2e-5


def build_module(c, dev):
    from fgnn_amd.mpnn import mp_conv_type, mp_conv_v2
    m = mp_conv_v2(c.nin, c.nou, c.net, bias=c.has_bias, bn=(c.bn != 'off'),
                   extension=mp_conv_type(c.ext), activation_fn='relu' if c.relu else None,
                   aggregtor=c.agg)
    m.load_state_dict(c.sd())
    m.train(c.bn == 'train')
    return m.to(dev)


@pytest.mark.parametrize('c', CASES, ids=[repr(c) for c in CASES])
def test_forward_matches_reference_golden(c, dev):
    m = build_module(c, dev)
    with torch.no_grad():
        y = m(c.t['x'].to(dev), c.t['idx'].to(dev), c.t['etype'].to(dev))
    assert y.shape == c.t['y'].shape
    assert H.rel_err(y, c.t['y']) <= TOL
    if c.bn == 'train':
        assert H.rel_err(m.bn.running_var, c.t['post_running_var']) <= TOL


@pytest.mark.parametrize('c', CASES, ids=[repr(c) for c in CASES])
def test_backward_matches_reference_golden(c, dev):
    m = build_module(c, dev)
    x = c.t['x'].to(dev).requires_grad_(True)
    et = c.t['etype'].to(dev).requires_grad_(True)
    y = m(x, c.t['idx'].to(dev), et)
    assert H.rel_err(y, c.t['y']) <= TOL
    y.backward(c.t['gy'].to(dev))
    # batch-statistics BatchNorm over B*M < 8 values is degenerate (over 2 values the true
    # gradient is exactly 0 and what is left is amplified rounding noise): looser bound there
    tol = 1e-3 if (c.bn == 'train' and c.B * c.M < 8) else 1e-4
    assert H.rel_err(x.grad, c.t['gx']) <= tol
    assert H.rel_err(et.grad, c.t['getype']) <= tol
    assert H.rel_err(m.filters.grad, c.t['gfilters']) <= tol
    if c.has_bias:
        assert H.rel_err(m.bias.grad, c.t['gbias']) <= tol


def _assert_argmax_names_a_maximiser(am, x, idx, et, W, nou, net, slack):
    """The uint8 argmax the forward hands to the backward must name, for every (sample, channel, destination), a
    neighbour whose f32 message (the oracle's per-edge tensor on the same inputs) is the maximum up to ``slack`` —
    an in-range but wrong neighbour would route gradients to the wrong edge while passing a value-only check."""
    k = idx.shape[2]
    am = am.cpu().long()
    assert int(am.max()) < k
    e = O.mp_conv({'filters': W}, '', x, idx, et, nou=nou, net=net, extension=0, aggregator=None, relu=False)   # [B,nou,M,k]
    chosen = e.gather(3, am)                                                    # am is [B,nou,M,1]
    gap = float((e.max(dim=3, keepdim=True)[0] - chosen).max())
    assert gap <= slack, (gap, slack)
    return gap


def _random_problem(seed, B, nin, nou, net, N, M, k, dev, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, nin, N, 1, generator=g)
    idx = torch.randint(0, N, (B, M, k), generator=g)
    et = torch.randn(B, net, M, k, generator=g)
    return x, idx, et, g


@pytest.mark.parametrize('ext,agg', [(0, 'max'), (0, 'softmax'), (2, 'max'), (1, 'mean'), (2, 'softmax')])
@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
def test_layouts_and_shared_graph_vs_oracle(ext, agg, layout, dev):
    """channels-last views and batch-stride-0 (expanded) graphs / edge weights give the same answer."""
    from fgnn_amd import _hip, ops
    B, nin, nou, net, N, k = 5, 12, 10, 4, 20, 3
    M = N if ext else 13
    x, idx, et, g = _random_problem(7 + ext, B, nin, nou, net, N, M, k, dev)
    idx = idx[:1].expand(B, -1, -1)                 # shared graph
    et = et[:1].expand(B, -1, -1, -1)               # shared edge weights
    R = nin if ext == 0 else 2 * nin
    sd = {'filters': torch.randn(R, nou * net, generator=g) * 0.3,
          'bias': torch.randn(nou, generator=g)}
    ref = O.mp_conv(sd, '', x, idx.contiguous(), et.contiguous(), nou=nou, net=net,
                    extension=ext, aggregator=agg, relu=False)
    xd = x.to(dev)
    if layout == 'channels_last':
        xd = xd.contiguous(memory_format=torch.channels_last)
    y, _ = ops.mpconv_forward_raw(xd, idx[:1].to(dev).expand(B, -1, -1),
                                  et[:1].to(dev).expand(B, -1, -1, -1), sd['filters'].to(dev),
                                  sd['bias'].to(dev), nou, net, ext, _hip.AGG_CODES[agg])
    assert H.rel_err(y, ref) <= TOL
    if layout == 'channels_last':
        assert y.stride(1) == 1          # output keeps the input's layout


@pytest.mark.parametrize('ext,agg,net', [(0, 'mean', 4), (1, 'mean', 16), (2, 'softmax', 5), (2, 'max', 3), (0, 'max', 7), (1, 'softmax', 1)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_generic_backward_is_bitwise_reproducible(ext, agg, net, dtype, dev):
    """The shape-generic backward (csrc/mpconv_bwd.hip: odd channel counts / edge-type counts, per-sample graphs, the `mean`
    aggregator, ...) used LDS and global float atomics until round 3.  Now every gradient element has one owner and a fixed
    summation order (CSR transpose of the sample's table in LDS, per-workgroup slabs folded in order): two runs give identical
    bits, and the values match the oracle's autograd (mp_nn.py:115-175)."""
    from fgnn_amd import _hip, ops
    B, nin, nou, N, k = 37, 12, 10, 23, 5
    M = N if ext else 17
    x, idx, et, g = _random_problem(31 + ext + net, B, nin, nou, net, N, M, k, dev)
    idx[:, 3, :] = idx[:, 3, :1]                       # a destination listening to one node k times (duplicates are legal)
    R = nin if ext == 0 else 2 * nin
    W, bias = torch.randn(R, nou * net, generator=g) * 0.3, torch.randn(nou, generator=g)
    gz = torch.randn(B, nou, M, 1, generator=g)
    xr, er = x.to(dtype).float(), et.to(dtype).float()

    def run():
        xd = xr.to(dev).to(dtype).requires_grad_(True)
        ed = er.to(dev).to(dtype).requires_grad_(True)
        Wd, bd = W.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
        z = ops.mpconv(xd, idx.to(dev), ed, Wd, bd, nou, net, ext, _hip.AGG_CODES[agg])
        z.backward(gz.to(dev).to(z.dtype))
        return xd.grad, ed.grad, Wd.grad, bd.grad, _hip.lib().fgnn_last_kernel().decode()

    a, b = run(), run()
    assert a[4].startswith('mpconv_bwd_kernel<'), a[4]
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)
    xo, eo = xr.clone().requires_grad_(True), er.clone().requires_grad_(True)
    sd = {'filters': W.clone().requires_grad_(True), 'bias': bias.clone().requires_grad_(True)}
    zo = O.mp_conv(sd, '', xo, idx, eo, nou=nou, net=net, extension=ext, aggregator=agg, relu=False)
    zo.backward(gz.to(dtype).float() if dtype == torch.bfloat16 else gz)
    tol = 1e-4 if dtype == torch.float32 else 2.0 ** -6
    assert H.rel_err(a[0].float(), xo.grad) <= tol and H.rel_err(a[1].float(), eo.grad) <= tol
    assert H.rel_err(a[2], sd['filters'].grad) <= tol and H.rel_err(a[3], sd['bias'].grad) <= tol


def test_bf16_storage_vs_oracle(dev):
    """bf16 x / etype / y with f32 accumulation: compare with the oracle run on the SAME
    bf16-rounded inputs; only the output rounding (2^-9 relative) differs."""
    from fgnn_amd import _hip, ops
    B, nin, nou, net, N, M, k = 4, 64, 64, 4, 96, 48, 6
    x, idx, et, g = _random_problem(3, B, nin, nou, net, N, M, k, dev)
    x, et = x.bfloat16(), et.bfloat16()
    sd = {'filters': torch.randn(nin, nou * net, generator=g) * 0.1, 'bias': torch.randn(nou, generator=g)}
    ref = O.mp_conv(sd, '', x.float(), idx, et.float(), nou=nou, net=net, extension=0,
                    aggregator='max', relu=True)
    y, _ = ops.mpconv_forward_raw(x.to(dev), idx.to(dev), et.to(dev), sd['filters'].to(dev),
                                  sd['bias'].to(dev), nou, net, 0, _hip.AGG_MAX, relu=True)
    assert y.dtype == torch.bfloat16
    err = (y.float().cpu() - ref).abs().max() / ref.abs().max()
    assert err <= 2.0 ** -8


def test_ldpc_sized_shapes_vs_oracle(dev):
    """The four operator shapes of the LDPC model at a batch the oracle finishes in seconds."""
    from fgnn_amd import _hip, ops
    shapes = [(64, 64, 4, 96, 48, 6), (64, 64, 4, 48, 96, 3), (64, 64, 1, 96, 1, 96),
              (64, 64, 1, 1, 96, 1), (64, 128, 4, 96, 48, 6), (128, 64, 4, 48, 96, 3)]
    for s, (nin, nou, net, N, M, k) in enumerate(shapes):
        x, idx, et, g = _random_problem(100 + s, 8, nin, nou, net, N, M, k, dev)
        sd = {'filters': torch.randn(nin, nou * net, generator=g) * 0.1,
              'bias': torch.randn(nou, generator=g)}
        ref = O.mp_conv(sd, '', x, idx, et, nou=nou, net=net, extension=0, aggregator='max', relu=False)
        y, am = ops.mpconv_forward_raw(x.to(dev), idx.to(dev), et.to(dev), sd['filters'].to(dev),
                                       sd['bias'].to(dev), nou, net, 0, _hip.AGG_MAX, want_argmax=True)
        assert H.rel_err(y, ref) <= TOL, (nin, nou, net, N, M, k)
        # f32 path: the named neighbour's message is the maximum to f32 rounding of the projection
        _assert_argmax_names_a_maximiser(am, x, idx, et, sd['filters'], nou, net, 1e-5 * float(ref.abs().max()))


def test_cpu_tensor_raises():
    from fgnn_amd import _hip, ops
    with pytest.raises(_hip.FgnnHipError):
        ops.mpconv_forward_raw(torch.zeros(1, 2, 3, 1), torch.zeros(1, 3, 2, dtype=torch.int64),
                               torch.zeros(1, 1, 3, 2), torch.zeros(2, 2), None, 2, 1, 0, 0)


@pytest.mark.parametrize('shape', [(64, 64, 4, 96, 48, 6), (64, 64, 4, 48, 96, 3), (64, 128, 4, 96, 48, 6),
                                   (128, 64, 4, 48, 96, 3), (64, 64, 1, 96, 8, 12), (128, 64, 4, 96, 48, 6),
                                   (64, 64, 4, 91, 47, 6), (64, 64, 4, 37, 95, 3), (64, 64, 4, 96, 1, 6)])
@pytest.mark.parametrize('agg', ['max', 'softmax'])
def test_bf16_mfma_kernel_vs_oracle(shape, agg, dev):
    """Channel-fastest bf16 inputs take the bf16-MFMA kernel (csrc/mpconv_fwd_b16.hip): x, etype,
    filters and the projected rows are bf16, sums f32.  Checked against the f32 oracle evaluated on the
    same bf16-rounded x / etype / filters; what remains is the rounding of P and of the output
    (2^-9 each) — bound 2^-6 of the output range, and the max-aggregator argmax must name a neighbour
    whose f32 message is within that bound of the true maximum."""
    from fgnn_amd import _hip, ops
    nin, nou, net, N, M, k = shape
    B = 6
    x, idx, et, g = _random_problem(11, B, nin, nou, net, N, M, k, dev)
    x, et = x.bfloat16(), et.bfloat16()
    W = (torch.randn(nin, nou * net, generator=g) * 0.1).bfloat16().float()
    sd = {'filters': W, 'bias': torch.randn(nou, generator=g)}
    ref = O.mp_conv(sd, '', x.float(), idx, et.float(), nou=nou, net=net, extension=0,
                    aggregator=agg, relu=False)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    etd = et.to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # edge-type fastest
    y, am = ops.mpconv_forward_raw(xd, idx.to(dev), etd, W.to(dev), sd['bias'].to(dev), nou, net, 0,
                                   _hip.AGG_CODES[agg], want_argmax=True)
    # per-sample tables keep the table-driven family away, M > 1 at one edge type the hyper-edge one
    kern = _hip.lib().fgnn_last_kernel().decode()
    assert kern.startswith('mpconv_fwd_b16_kernel<%d, %d, ' % (net, _hip.AGG_CODES[agg])), kern
    assert y.dtype == torch.bfloat16 and y.stride(1) == 1
    err = float((y.float().cpu() - ref).abs().max() / ref.abs().max())
    assert err <= 2.0 ** -6, err
    if agg == 'max':
        # near-tie rule: the bf16 rounding of P may prefer another neighbour than f32 does, but only one whose f32
        # message is within the same 2^-6 of the output range of the true maximum
        rng = float((ref - sd['bias'][None, :, None, None]).abs().max())
        _assert_argmax_names_a_maximiser(am, x.float(), idx, et.float(), W, nou, net, 2.0 ** -6 * rng)


@pytest.mark.parametrize('shape', [(64, 64, 96, 48, 6), (64, 64, 48, 96, 3), (64, 128, 96, 48, 6), (64, 128, 48, 96, 3),
                                   (128, 64, 96, 48, 6), (128, 64, 48, 96, 3), (64, 64, 40, 20, 5), (64, 64, 91, 47, 6),
                                   (64, 64, 37, 95, 3), (64, 128, 50, 33, 4)],
                         ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('shared', [False, True], ids=['pergraph', 'sharedgraph'])
def test_bf16_mfma_backward_vs_routed_reference(shape, shared, dev):
    """bf16 channel-fastest parity-check calls (4 edge types) take csrc/mpconv_bwd_b16.hip: bf16 matrix cores
    for the P / dx / dW projections, P and dP rounded to bf16 in LDS.  Checked against torch autograd through
    the SAME routing (the forward's own argmax) on the same bf16-rounded x / etype / gz, f32 arithmetic:
    what remains is the bf16 rounding of P, dP and of the bf16 outputs -> 2^-6 of each gradient's range."""
    from fgnn_amd import _hip, ops
    nin, nou, N, M, k = shape
    net, B = 4, 11
    g = torch.Generator().manual_seed(21 + N + nou)
    x = torch.randn(B, nin, N, 1, generator=g).bfloat16()
    idx = torch.randint(0, N, (1 if shared else B, M, k), generator=g)
    if shared:
        idx = idx.expand(B, -1, -1)
    et = torch.randn(B, M, k, net, generator=g).bfloat16()                  # edge-type fastest in memory
    W = torch.randn(nin, nou * net, generator=g) * 0.1
    bias = torch.randn(nou, generator=g)
    gz = torch.randn(B, nou, M, 1, generator=g).bfloat16()
    xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    etd = et.to(dev).permute(0, 3, 1, 2).requires_grad_(True)               # logical [B,net,M,k]
    idxd = idx.to(dev) if not shared else idx[:1].to(dev).expand(B, -1, -1)
    Wd, bd = W.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    z = ops.mpconv(xd, idxd, etd, Wd, bd, nou, net, 0, _hip.AGG_MAX)
    _, am = ops.mpconv_forward_raw(xd.detach(), idxd, etd.detach(), W.to(dev), bias.to(dev), nou, net, 0,
                                   _hip.AGG_MAX, want_argmax=True)
    z.backward(gz.to(dev))
    kern = _hip.lib().fgnn_last_kernel().decode()       # (a random table whose in-degree happens to fit goes to the table-driven family; test_mpconv_sg_irregular_gpu.py builds such tables deliberately)
    assert 'mpconv_bwd_b16' in kern or 'mpconv_bwd_ws' in kern, kern
    xr = x.float().detach().clone().requires_grad_(True)
    er = et.float().detach().clone().requires_grad_(True)                    # [B,M,k,net]
    Wr, br = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    P = torch.einsum('bcn,cq->bnq', xr[..., 0], Wr).reshape(B, N, nou, net)
    E = (P[torch.arange(B)[:, None, None], idx] * er[:, :, :, None, :]).sum(-1)          # [B,M,k,nou]
    sel = am.cpu().long()[..., 0].permute(0, 2, 1)[:, :, None, :]                        # [B,M,1,nou]
    zr = E.gather(2, sel)[:, :, 0, :].permute(0, 2, 1)[..., None] + br[None, :, None, None]
    zr.backward(gz.float())
    tol = 2.0 ** -6
    assert H.rel_err(xd.grad.float(), xr.grad) <= tol
    assert H.rel_err(etd.grad.float(), er.grad.permute(0, 3, 1, 2)) <= tol
    assert H.rel_err(Wd.grad, Wr.grad) <= tol
    assert H.rel_err(bd.grad, br.grad) <= tol


HYPER_SHAPES = [(64, 64, 96, 1, 96), (64, 64, 1, 96, 1), (64, 128, 96, 1, 96), (64, 128, 1, 96, 1),
                (128, 64, 96, 1, 96), (128, 64, 1, 96, 1), (64, 64, 40, 1, 130), (64, 64, 1, 7, 1)]


@pytest.mark.parametrize('shape', [(64, 64, 96, 1, 96), (64, 64, 1, 96, 1), (64, 128, 96, 1, 96), (64, 128, 1, 96, 1),
                                   (128, 64, 96, 1, 96), (128, 64, 1, 96, 1), (64, 64, 40, 1, 130), (64, 64, 1, 7, 1)],
                         ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('agg', ['max', 'softmax', 'mean'])
def test_bf16_hyper_edge_forward_vs_oracle(shape, agg, dev):
    """bf16 channel-fastest hyper-factor calls take csrc/mpconv_fwd_hyper.hip (one wave per sample).  Same
    check as the bf16-MFMA kernel: f32 oracle on the same bf16-rounded x / etype / filters, bound 2^-6 of the
    output range (P and the output are rounded to bf16); bias, folded affine and ReLU are exercised too."""
    from fgnn_amd import _hip, ops
    nin, nou, N, M, k = shape
    B = 13
    g = torch.Generator().manual_seed(31 + N + nou)
    x = torch.randn(B, nin, N, 1, generator=g).bfloat16()
    idx = torch.randint(0, N, (B, M, k), generator=g)
    et = (torch.rand(B, 1, M, k, generator=g) + 0.5).bfloat16()
    W = (torch.randn(nin, nou, generator=g) * 0.1).bfloat16().float()
    bias = torch.randn(nou, generator=g)
    scale, shift = torch.rand(nou, generator=g) + 0.5, torch.randn(nou, generator=g)
    ref = O.mp_conv({'filters': W, 'bias': bias}, '', x.float(), idx, et.float(), nou=nou, net=1, extension=0,
                    aggregator=agg, relu=False)
    ref = torch.relu(ref * scale[None, :, None, None] + shift[None, :, None, None])
    xd = x.to(dev).contiguous(memory_format=torch.channels_last)
    y, am = ops.mpconv_forward_raw(xd, idx.to(dev), et.to(dev), W.to(dev), bias.to(dev), nou, 1, 0,
                                   _hip.AGG_CODES[agg], post_scale=scale.to(dev), post_shift=shift.to(dev),
                                   relu=True, want_argmax=True)
    assert ('fanin' if M == 1 else 'fanout') in _hip.lib().fgnn_last_kernel().decode()
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape
    err = float((y.float().cpu() - ref).abs().max() / ref.abs().max())
    assert err <= 2.0 ** -6, err
    if agg == 'max':
        pre = O.mp_conv({'filters': W}, '', x.float(), idx, et.float(), nou=nou, net=1, extension=0, aggregator='max',
                        relu=False)
        _assert_argmax_names_a_maximiser(am, x.float(), idx, et.float(), W, nou, 1, 2.0 ** -6 * float(pre.abs().max()))


@pytest.mark.parametrize('shape', HYPER_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_hyper_edge_backward_vs_routed_reference(shape, layout, dtype, dev):
    """Constant-etype hyper-factor calls (one destination of high degree / one source fanned out) take
    csrc/mpconv_bwd_hyper.hip.  Checked against torch autograd through the same routing: the forward's
    own argmax selects the neighbour (so a bf16 forward that picks another near-tie winner than the f32
    oracle does not blur what is being tested), and — in f32 — against the oracle's autograd too.
    Duplicate neighbours, non-unit edge weights and a batch that is not a multiple of the 8 waves of a
    workgroup are all in."""
    from fgnn_amd import _hip, ops
    nin, nou, N, M, k = shape
    B = 19
    g = torch.Generator().manual_seed(5 + N + k)
    x = torch.randn(B, nin, N, 1, generator=g).to(dtype)
    idx = torch.randint(0, N, (B, M, k), generator=g)
    et = (torch.rand(B, 1, M, k, generator=g) + 0.5).to(dtype)
    W = torch.randn(nin, nou, generator=g) * 0.1
    bias = torch.randn(nou, generator=g)
    gz = torch.randn(B, nou, M, 1, generator=g).to(dtype)
    xd = x.to(dev)
    if layout == 'channels_last':
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_(True)
    Wd, bd = W.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    z = ops.mpconv(xd, idx.to(dev), et.to(dev), Wd, bd, nou, 1, 0, _hip.AGG_MAX)
    # the argmax the forward recorded (re-run raw: the autograd Function keeps its own copy)
    _, am = ops.mpconv_forward_raw(xd.detach(), idx.to(dev), et.to(dev), W.to(dev), bias.to(dev), nou, 1, 0,
                                   _hip.AGG_MAX, want_argmax=True)
    z.backward(gz.to(dev))
    assert ('fanin' if M == 1 else 'fanout') in _hip.lib().fgnn_last_kernel().decode()
    # routed reference in f32 on the CPU
    xr = x.float().detach().clone().requires_grad_(True)
    Wr, br = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    P = torch.einsum('bcn,co->bno', xr[..., 0], Wr)                                 # [B,N,nou]
    E = P[torch.arange(B)[:, None, None], idx] * et.float()[:, 0, :, :, None]       # [B,M,k,nou]
    sel = am.cpu().long()[..., 0].permute(0, 2, 1)[:, :, None, :]                   # [B,M,1,nou]
    zr = E.gather(2, sel)[:, :, 0, :].permute(0, 2, 1)[..., None] + br[None, :, None, None]
    zr.backward(gz.float())
    tol = 2e-5 if dtype == torch.float32 else 2.0 ** -7
    assert H.rel_err(xd.grad.float(), xr.grad) <= tol
    assert H.rel_err(Wd.grad, Wr.grad) <= tol
    assert H.rel_err(bd.grad, br.grad) <= tol
    if dtype == torch.float32:
        xo = x.detach().clone().requires_grad_(True)
        sd = {'filters': W.clone().requires_grad_(True), 'bias': bias.clone().requires_grad_(True)}
        zo = O.mp_conv(sd, '', xo, idx, et, nou=nou, net=1, extension=0, aggregator='max', relu=False)
        assert H.rel_err(z, zo) <= TOL
        zo.backward(gz)
        assert H.rel_err(xd.grad, xo.grad) <= 1e-4
        assert H.rel_err(Wd.grad, sd['filters'].grad) <= 1e-4


@pytest.mark.parametrize('shape', [(64, 64, 96, 96), (64, 128, 96, 96), (128, 64, 96, 96), (64, 64, 40, 130), (64, 64, 96, 7)],
                         ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('tables', ['ldpc', 'shared', 'per_sample'])
def test_bf16_fan_in_backward_many_samples_per_wave_vs_routed_reference(shape, tables, dev):
    """csrc/mpconv_bwd_hyper.hip::mpconv_bwd_fanin_kernel (bf16 channel-fastest states, one destination of degree k): at a batch
    where the grid is capped and every wave owns several samples, with the LDPC hyper-factor's own tables (identity list, unit
    weights, both stride-0 over the batch: train_ldpc.py:40-46), a random table shared by the batch and per-sample tables; dx
    (zeros of the rows nobody routed to included), dW and dbias against torch autograd through the forward's own routing; the
    kernel ran; bit-reproducible."""
    from fgnn_amd import _hip, ops
    nin, nou, N, k = shape
    B = 2500
    g = torch.Generator().manual_seed(11 + N + k + nou)
    x = torch.randn(B, nin, N, 1, generator=g).to(torch.bfloat16)
    if tables == 'ldpc' and k == N:
        idx = torch.arange(N).reshape(1, 1, N).expand(B, -1, -1)
        et = torch.ones(1, 1, 1, k, dtype=torch.bfloat16).expand(B, -1, -1, -1)
    elif tables == 'per_sample':
        idx = torch.randint(0, N, (B, 1, k), generator=g)
        et = (torch.rand(B, 1, 1, k, generator=g) + 0.5).to(torch.bfloat16)
    else:
        idx = torch.randint(0, N, (1, 1, k), generator=g).expand(B, -1, -1)
        et = (torch.rand(1, 1, 1, k, generator=g) + 0.5).to(torch.bfloat16).expand(B, -1, -1, -1)
    W = torch.randn(nin, nou, generator=g) * 0.1
    bias = torch.randn(nou, generator=g)
    gz = torch.randn(B, nou, 1, 1, generator=g).to(torch.bfloat16)
    idx_d, et_d = idx.to(dev), et.to(dev)
    if tables != 'per_sample':           # (.to() materialises an expanded tensor: restore the stride-0 batch axis)
        idx_d, et_d = idx[:1].to(dev).expand(B, -1, -1), et[:1].to(dev).expand(B, -1, -1, -1)
    _, am = ops.mpconv_forward_raw(x.to(dev).contiguous(memory_format=torch.channels_last), idx_d, et_d, W.to(dev), bias.to(dev), nou, 1, 0,
                                   _hip.AGG_MAX, want_argmax=True)
    outs = []
    for _ in range(2):
        xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        Wd, bd = W.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
        z = ops.mpconv(xd, idx_d, et_d, Wd, bd, nou, 1, 0, _hip.AGG_MAX)
        z.backward(gz.to(dev))
        assert _hip.lib().fgnn_last_kernel().decode().startswith('mpconv_bwd_fanin_kernel'), _hip.lib().fgnn_last_kernel().decode()
        outs.append((xd.grad.clone(), Wd.grad.clone(), bd.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    xr = x.float().detach().clone().requires_grad_(True)
    Wr, br = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    P = torch.einsum('bcn,co->bno', xr[..., 0], Wr)                                 # [B,N,nou]
    E = P[torch.arange(B)[:, None, None], idx] * et.float()[:, 0, :, :, None]       # [B,1,k,nou]
    sel = am.cpu().long()[..., 0].permute(0, 2, 1)[:, :, None, :]                   # [B,1,1,nou]
    zr = E.gather(2, sel)[:, :, 0, :].permute(0, 2, 1)[..., None] + br[None, :, None, None]
    zr.backward(gz.float())
    gxd, gWd, gbd = outs[0]
    assert H.rel_err(gxd.float(), xr.grad) <= 2.0 ** -7
    assert H.rel_err(gWd, Wr.grad) <= 2.0 ** -7
    assert H.rel_err(gbd, br.grad) <= 2.0 ** -7
    # rows nobody routed to are exact zeros
    assert bool(((xr.grad == 0) <= (gxd.float().cpu() == 0)).all())


@pytest.mark.parametrize('cin,cout', [(64, 64), (2, 64), (7, 64), (96, 64), (64, 256), (256, 64), (256, 256),
                                      (128, 1), (64, 4), (100, 12), (7, 128), (256, 3)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_pointwise_conv_gradients_vs_torch(cin, cout, dtype, dev):
    """PointwiseConv2d (GEMM forward, hand-written split-rows weight-gradient kernel) against
    torch.nn.Conv2d autograd in f32 on the same (rounded) inputs."""
    from fgnn_amd.mpnn import PointwiseConv2d
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    B, N = 7, 50
    x = torch.randn(B, cin, N, 1, generator=g).to(dtype)
    ref = torch.nn.Conv2d(cin, cout, 1)
    mine = PointwiseConv2d(cin, cout, 1)
    mine.load_state_dict(ref.state_dict())
    gy = torch.randn(B, cout, N, 1, generator=g).to(dtype)
    xr = x.detach().float().clone().requires_grad_(True)
    ref(xr).backward(gy.float())
    mine = mine.to(dev)
    xm = x.detach().clone().to(dev).requires_grad_(True)
    ym = mine(xm)
    ym.backward(gy.to(dev))
    tol = 1e-4 if dtype == torch.float32 else 2e-2
    assert H.rel_err(ym.float(), ref(xr)) <= tol
    assert H.rel_err(mine.weight.grad, ref.weight.grad) <= tol
    assert H.rel_err(mine.bias.grad, ref.bias.grad) <= tol
    assert H.rel_err(xm.grad.float(), xr.grad) <= tol


@pytest.mark.parametrize('cin,cout', [(64, 64), (64, 128), (128, 64), (64, 256), (256, 64), (256, 256), (192, 128)])
@pytest.mark.parametrize('rows', [(3, 37), (64, 96)], ids=['r111', 'r6144'])
def test_linear_forward_with_fused_batch_statistics(cin, cout, rows, dev):
    """bf16 node-wise map through csrc/linear_fwd_b16.hip, alone and with the BatchNorm statistics taken from
    its epilogue: (a) the GEMM against torch in f32 on the same bf16 inputs (only the output rounding differs),
    (b) conv -> BatchNorm+LeakyReLU with the fused statistics against the same modules with the statistics pass
    (identical up to computing mean / variance from the unrounded f32 accumulators)."""
    from fgnn_amd.mpnn import PointwiseConv2d
    from fgnn_amd.mpnn.pointwise import BatchNormAct2d, BnHandoff
    B, N = rows
    g = torch.Generator().manual_seed(cin + 7 * cout + N)
    x = torch.randn(B, cin, N, 1, generator=g).bfloat16().to(dev).contiguous(memory_format=torch.channels_last)
    conv = PointwiseConv2d(cin, cout, 1).to(dev)
    with torch.no_grad():
        y = conv(x)
    assert y.dtype == torch.bfloat16
    ref = torch.nn.functional.conv2d(x.float(), conv.weight, conv.bias)
    assert H.rel_err(y.float(), ref) <= 2.0 ** -7
    bn_a, bn_b = BatchNormAct2d(cout, slope=0.01).to(dev).train(), BatchNormAct2d(cout, slope=0.01).to(dev).train()
    with torch.no_grad():
        bn_a.weight.uniform_(0.5, 1.5); bn_a.bias.uniform_(-0.5, 0.5)
    bn_b.load_state_dict(bn_a.state_dict())
    xa = x.detach().clone().requires_grad_(True)
    xb = x.detach().clone().requires_grad_(True)
    h = BnHandoff.of(bn_a)
    ya = bn_a(conv(xa, bn=h), handoff=h)                 # statistics from the GEMM epilogue, finalised by the GEMM's last workgroup
    yb = bn_b(conv(xb))                                  # statistics pass over the bf16 output
    assert H.rel_err(ya.float(), yb.float()) <= 2.0 ** -6
    assert H.rel_err(bn_a.running_mean, bn_b.running_mean) <= 1e-3
    assert H.rel_err(bn_a.running_var, bn_b.running_var) <= 1e-3
    gy = torch.randn_like(ya)
    conv.zero_grad()
    ya.backward(gy)
    ga = xa.grad.float().clone()
    yb.backward(gy)
    # elements whose pre-activation sits within rounding of the LeakyReLU kink take the other slope in one of
    # the two runs (their gradient then differs by O(1)): compare in the mean, not the max
    gb = xb.grad.float()
    # (256 inputs: the reference run's map is the library GEMM — see test_iid_mapping_in_as_one_kernel — and a few more elements sit on the kink)
    assert float((ga - gb).abs().mean()) <= (1e-2 if cin <= 128 else 2e-2) * float(gb.abs().mean())


@pytest.mark.parametrize('C,N', [(64, 96), (256, 48), (128, 96), (10, 7), (64, 2)])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_instance_norm_kernel_vs_torch(C, N, relu, dtype, dev):
    """Fused InstanceNorm(+ReLU) kernel (csrc/instnorm.hip) forward and backward against
    torch.nn.functional.instance_norm in f32 on the same inputs."""
    from fgnn_amd.mpnn import NodeInstanceNorm
    g = torch.Generator().manual_seed(C * 100 + N)
    B = 5
    x = (torch.randn(B, C, N, 1, generator=g) * 2 + 0.5).to(dtype)
    gy = torch.randn(B, C, N, 1, generator=g).to(dtype)
    xr = x.detach().float().clone().requires_grad_(True)
    ref = torch.nn.functional.instance_norm(xr, eps=1e-5)
    if relu:
        ref = torch.relu(ref)
    ref.backward(gy.float())
    xm = x.detach().clone().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = NodeInstanceNorm(relu=relu)(xm)
    y.backward(gy.to(dev))
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    assert H.rel_err(y.float(), ref) <= tol
    assert H.rel_err(xm.grad.float(), xr.grad) <= tol * 5


@pytest.mark.parametrize('N,B', [(96, 5), (48, 3), (128, 2), (2, 4), (37, 700)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_classifier_instnorm_relu_dot_kernel_vs_torch(N, B, dtype, dev):
    """The classifier's closing pair InstanceNorm2d -> ReLU -> Conv2d(128, 1, 1) (factor_mpnn_sp.py:104-108) as one kernel
    (csrc/instnorm.hip: instnorm_dot_kernel) against the same three torch ops in f32: logits, input gradient, the map's weight and
    bias gradients (B = 700: more samples than backward workgroups, so the grid-stride walk and the partial-row fold are on)."""
    from fgnn_amd import ops
    from fgnn_amd.mpnn.pointwise import instnorm_relu_dot, PointwiseConv2d
    g = torch.Generator().manual_seed(N * 10 + B)
    x = (torch.randn(B, 128, N, 1, generator=g) * 2 + 0.5).to(dtype)
    gout = torch.randn(B, 1, N, 1, generator=g).to(dtype)
    conv = PointwiseConv2d(128, 1, 1, bias=True)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(1, 128, 1, 1, generator=g) * 0.2)
        conv.bias.fill_(0.3)
    xr = x.detach().float().clone().requires_grad_(True)
    wr, br = conv.weight.detach().clone().requires_grad_(True), conv.bias.detach().clone().requires_grad_(True)
    ref = torch.nn.functional.conv2d(torch.relu(torch.nn.functional.instance_norm(xr, eps=1e-5)), wr, br)
    ref.backward(gout.float())
    conv = conv.to(dev)
    xm = x.detach().clone().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    rec = []
    ops.TIMER = type('T', (), {'run': staticmethod(lambda sym, nb, nf, launch, use_note=True, **kw: (rec.append(sym), launch()))})()
    try:
        out = instnorm_relu_dot(xm, conv)
        out.backward(gout.to(dev))
    finally:
        ops.TIMER = None
    assert rec == ['instnorm_dot_kernel<fwd>', 'instnorm_dot_kernel<bwd>'], rec
    tol = 2e-5 if dtype == torch.float32 else 1e-2
    assert out.shape == ref.shape and out.dtype == dtype
    assert H.rel_err(out.float(), ref) <= tol
    assert H.rel_err(xm.grad.float(), xr.grad) <= tol * 5
    assert H.rel_err(conv.weight.grad, wr.grad) <= tol
    assert H.rel_err(conv.bias.grad, br.grad) <= tol
    with torch.no_grad():                                    # the no-grad form (inference) is the same launch
        assert torch.equal(instnorm_relu_dot(xm.detach(), conv), out.detach())
    # shapes outside the kernel's: None, the caller runs the staged modules
    assert instnorm_relu_dot(torch.zeros(2, 64, N, 1, device=dev), conv) is None
    assert instnorm_relu_dot(xm.detach().cpu(), conv.cpu()) is None


@pytest.mark.parametrize('K,C', [((64, 0, 0), 64), ((64, 64, 64), 64), ((64, 128, 64), 64), ((64, 256, 64), 128), ((64, 256, 64), 256),
                                 ((64, 128, 64), 256), ((64, 64, 0), 128), ((0, 256, 0), 256), ((64, 0, 64), 64), ((64, 256, 0), 256)])
@pytest.mark.parametrize('nadd', [0, 2, 3])
def test_linear_multi_kernel_vs_torch(K, C, nadd, dev):
    """csrc/linear_fwd_b16.hip::linear_multi_b16_kernel — y = sum_s x_s W_s + addends, the gradient of a FactorNN state with several
    consumers as one K-concatenated product (ops.FanBox) — against the same sum of f32 matmuls on the same bf16 operands; R not a
    multiple of the 16-row tile; wide products run as two output-channel slices."""
    import ctypes
    from fgnn_amd import _hip
    L = _hip.lib()
    R = 1000 + 7
    g = torch.Generator().manual_seed(sum(K) + C + nadd)
    xs = [torch.randn(R, k, generator=g).bfloat16().to(dev) if k else None for k in K]
    Ws = [(torch.randn(k, C, generator=g) * 0.1).to(dev) if k else None for k in K]
    adds = [torch.randn(R, C, generator=g).bfloat16().to(dev) for _ in range(nadd)]
    ks = (ctypes.c_int32 * 3)(*K)
    assert L.fgnn_linear_multi_supported(R, ks, C) == 1
    y = torch.empty(R, C, device=dev, dtype=torch.bfloat16)
    P = _hip._ptr
    arr = lambda ts: (ctypes.c_void_p * 3)(*([P(t) for t in ts] + [None] * (3 - len(ts))))
    _hip.check(L.fgnn_linear_multi_forward(arr(xs), ks, arr(Ws), arr(adds), P(y), R, C, _hip.stream_ptr()))
    ref = sum(x.float() @ w.bfloat16().float() for x, w in zip(xs, Ws) if x is not None)
    for a in adds:
        ref = ref + a.float()
    err = float((y.float() - ref).abs().max() / ref.abs().max())
    assert err <= 2.0 ** -7, err
    bad = (ctypes.c_int32 * 3)(0, 64, 64)
    assert L.fgnn_linear_multi_supported(R, bad, C) == 0 and L.fgnn_linear_multi_supported(R, ks, 96) == 0


@pytest.mark.parametrize('C', [64, 128, 256, 8, 96])
@pytest.mark.parametrize('slope', [0.0, 0.01, 1.0])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_batchnorm_act_kernel_vs_torch(C, slope, dtype, dev):
    """Fused train-mode BatchNorm + (Leaky)ReLU (csrc/bnact.hip; C=96 takes the torch fallback) against
    torch.nn.BatchNorm2d + activation in f32: output, input/affine gradients, running statistics."""
    from fgnn_amd.mpnn import BatchNormAct2d
    g = torch.Generator().manual_seed(C)
    B, N = 9, 40
    x = (torch.randn(B, C, N, 1, generator=g) * 1.5 + 0.7).to(dtype)
    gy = torch.randn(B, C, N, 1, generator=g).to(dtype)
    ref = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        ref.weight.copy_(1 + 0.3 * torch.randn(C, generator=g))
        ref.bias.copy_(0.3 * torch.randn(C, generator=g))
    mine = BatchNormAct2d(C, slope=slope)
    mine.load_state_dict(ref.state_dict())
    act = (lambda t: t) if slope == 1.0 else (torch.relu if slope == 0.0 else
                                              (lambda t: torch.nn.functional.leaky_relu(t, slope)))
    xr = x.detach().float().clone().requires_grad_(True)
    yr = act(ref(xr))
    yr.backward(gy.float())
    mine = mine.to(dev).train()
    xm = x.detach().clone().to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ym = mine(xm)
    ym.backward(gy.to(dev))
    tol = 5e-5 if dtype == torch.float32 else 2e-2
    assert H.rel_err(ym.float(), yr) <= tol
    assert H.rel_err(xm.grad.float(), xr.grad) <= tol * 4
    assert H.rel_err(mine.weight.grad, ref.weight.grad) <= tol * 4
    assert H.rel_err(mine.bias.grad, ref.bias.grad) <= tol * 4
    assert H.rel_err(mine.running_mean, ref.running_mean) <= tol
    assert H.rel_err(mine.running_var, ref.running_var) <= tol * 2
    assert int(mine.num_batches_tracked) == 1


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('layout', ['nchw', 'channels_last'])
def test_fan_out_and_add_n_match_plain_autograd(dtype, layout, dev):
    """ops.fan_out / ops.add_n (csrc/sum_n.hip: one n-input pass) against ordinary autograd on the same graph:
    forward sum identical in f32 (same left-to-right order), gradients equal up to the summation order."""
    from fgnn_amd import ops
    g = torch.Generator().manual_seed(4)
    mk = lambda: torch.randn(5, 64, 12, 1, generator=g).to(dtype).to(dev)
    x, p, q = mk(), mk(), mk()
    if layout == 'channels_last':
        x, p, q = [t.contiguous(memory_format=torch.channels_last) for t in (x, p, q)]
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    w = [mk() for _ in range(4)]
    if layout == 'channels_last':
        w = [t.contiguous(memory_format=torch.channels_last) for t in w]
    c = ops.fan_out(xa, 4)
    ya = ops.add_n([c[0] * w[0], c[1] * w[1], c[2] * w[2] + p, c[3]])
    yb = ((xb * w[0] + xb * w[1]) + (xb * w[2] + p)) + xb
    tol = 0.0 if dtype == torch.float32 else 2.0 ** -7
    assert H.rel_err(ya.float(), yb.float()) <= tol
    gy = mk()
    ya.backward(gy)
    yb.backward(gy)
    assert H.rel_err(xa.grad.float(), xb.grad.float()) <= (1e-6 if dtype == torch.float32 else 2.0 ** -6)


@pytest.mark.parametrize('shape', [(96, 48, 6), (48, 96, 3)], ids=['v2f', 'f2v'])
@pytest.mark.parametrize('B', [5, 300, 1100])
def test_bf16_forward_statistics_epilogue_feeds_batchnorm(shape, B, dev):
    """Training-mode mp_conv_v2 (64 -> 64, 4 edge types): the operator's forward kernel leaves the batch statistics of
    its stored output for the BatchNorm behind it (mp_nn.py:170) — same output, running statistics and gradients as
    with BatchNorm's own reduction pass over z."""
    import fgnn_amd
    from fgnn_amd import _hip, ops
    from fgnn_amd.mpnn import mp_conv_type, mp_conv_v2
    N, M, k = shape
    g = torch.Generator().manual_seed(B + N)
    x = torch.randn(B, N, 1, 64, generator=g).bfloat16().to(dev).permute(0, 3, 1, 2)
    idx = torch.randint(0, N, (B, M, k), generator=g).to(dev)
    et = torch.randn(B, M, k, 4, generator=g).bfloat16().to(dev).permute(0, 3, 1, 2)
    gy = torch.randn(B, M, 1, 64, generator=g).bfloat16().to(dev).permute(0, 3, 1, 2)

    def run(epilogue):
        torch.manual_seed(7)
        m = mp_conv_v2(64, 64, 4, extension=mp_conv_type.NO_EXTENSION, aggregtor='max').to(dev).train()
        xx = x.detach().clone().requires_grad_(True)
        ops.STATS_EPILOGUE = epilogue
        try:
            y = m(xx, idx, et)
        finally:
            ops.STATS_EPILOGUE = True
        y.backward(gy)
        return y.detach().float(), m.bn.running_mean.clone(), m.bn.running_var.clone(), xx.grad.float(), m.filters.grad.clone()

    a = run(True)
    b = run(False)
    assert H.rel_err(a[0], b[0]) <= 2.0 ** -7 and H.rel_err(a[3], b[3]) <= 2.0 ** -6
    assert H.rel_err(a[1], b[1]) <= 1e-5 and H.rel_err(a[2], b[2]) <= 1e-4 and H.rel_err(a[4], b[4]) <= 2e-3
    # the epilogue is really what ran: no bn_stats launch for this BatchNorm
    ops.TIMER = ops.KernelTimer()
    try:
        run(True)
        names = set(ops.TIMER.summary())
    finally:
        ops.TIMER = None
    assert not any(n.startswith('bn_stats') for n in names), names


@pytest.mark.parametrize('R,cin,cout', [(61440, 128, 64), (61440, 256, 256), (5001, 512, 256), (2048, 64, 128), (30720, 132, 68), (4096, 1024, 16),
                                         (3840, 64, 64), (3900, 64, 64), (3840, 256, 64), (2050, 64, 256), (15360, 64, 64)])
def test_f32_blocked_weight_gradient_vs_torch(R, cin, cout, dev):
    """csrc/linear_wgrad_f32.hip (f32 node-wise maps of the synthetic-PGM models) through fgnn_linear_wgrad: against a float64
    torch product, accumulating into gW / gb, and bit-identical on a second run (slab fold in a fixed order)."""
    import ctypes
    from fgnn_amd import _hip, ops
    L = _hip.lib()
    g = torch.Generator().manual_seed(R + cin)
    x = torch.randn(R, cin, generator=g).to(dev)
    gy = torch.randn(R, cout, generator=g).to(dev)
    ref_w = (gy.double().t() @ x.double())
    ref_b = gy.double().sum(0)
    kernel = _hip.invoke('fgnn_linear_wgrad_kernel', R, cin, cout, _hip.dtype_code(x), x.data_ptr() & 15, gy.data_ptr() & 15)
    assert kernel.startswith(b'linear_wgrad_f32q_kernel<'), kernel       # the family this test is about, not the general kernel
    outs = []
    for _ in range(2):
        gw = torch.ones(cout, cin, device=dev)
        gb = torch.full((cout,), 2.0, device=dev)
        ws = ops._workspace(dev, int(L.fgnn_linear_wgrad_workspace_bytes(R, cin, cout)))
        _hip.check(L.fgnn_linear_wgrad(_hip._ptr(x), _hip._ptr(gy), R, cin, cout, _hip.dtype_code(x), _hip._ptr(gw), _hip._ptr(gb),
                                       _hip._ptr(ws), ws.numel() * 4, _hip.stream_ptr()))
        outs.append((gw.clone(), gb.clone()))
    gw, gb = outs[0]
    assert float(((gw.double() - 1.0) - ref_w).abs().max()) <= 2e-5 * float(ref_w.abs().max())
    assert float(((gb.double() - 2.0) - ref_b).abs().max()) <= 2e-5 * float(ref_b.abs().max())
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize('R,cin,couts', [(6144, 64, (64, 64, 64)), (6149, 64, (64, 128, 64)), (12288, 128, (64, 256, 64)), (6144, 256, (64, 64)),
                                          (6144, 256, (64, 128, 64)), (3000, 128, (64, 64, 64)), (393216, 64, (64, 64)), (40, 64, (64, 64, 64)),
                                          (6144, 64, (256,)),
                                          # the LDS-staged kernel (8 / 16 slices): partial last stages, fewer stages than workgroups / than the
                                          # pipeline is deep, one wide map alone, 128- and 256-byte rows beside 512-byte ones
                                          (6149, 256, (64, 128, 64)), (4101, 256, (64, 64)), (2048 + 37, 256, (256,)), (9000, 128, (256,)),
                                          (8192 + 31, 256, (128,)), (12288 + 5, 128, (64, 256, 64)), (2049, 256, (128, 128)), (70000, 256, (256,)),
                                          # stages that are not a multiple of 16 KB (waves issue different numbers of DMA instructions)
                                          (6144 + 3, 128, (64, 256)), (5000, 256, (64, 128)), (4100, 128, (64, 64, 64))])
@pytest.mark.parametrize('deferred', [False, True])
def test_bf16_weight_gradients_of_several_maps_over_one_state(R, cin, couts, deferred, dev):
    """fgnn_linear_wgrad_multi (csrc/linear_wgrad_b16.hip: the weight / bias gradients of the node-wise maps that consume ONE layer
    state — factor_mpnn_sp.py:136-168 — in one pass over its rows): every map's gW / gb against a float64 product on the same bf16
    operands, ACCUMULATED into, equal to what fgnn_linear_wgrad gives map by map (same grid: same sums), with immediate and with
    recorded folds (csrc/fold_batch.hip), bit-identical on a second run; R not a multiple of the 32-row blocks; shapes outside
    the family are refused by the workspace query."""
    import ctypes
    from fgnn_amd import _hip, ops
    L = _hip.lib()
    P = _hip._ptr
    g = torch.Generator().manual_seed(R + cin + sum(couts))
    x = torch.randn(R, cin, generator=g).to(dev).to(torch.bfloat16)
    gys = [torch.randn(R, c, generator=g).to(dev).to(torch.bfloat16) for c in couts]
    n = len(couts)
    cc = (ctypes.c_int32 * n)(*couts)
    nb = int(L.fgnn_linear_wgrad_multi_workspace_bytes(R, cin, n, cc))
    assert nb > 0

    def run(multi):
        gws = [torch.ones(c, cin, device=dev) for c in couts]
        gbs = [torch.full((c,), 2.0, device=dev) for c in couts]
        keep = []
        L.fgnn_fold_discard()
        L.fgnn_fold_defer(1 if deferred else 0)
        try:
            if multi:
                ws = torch.empty(nb // 4, device=dev)
                keep.append(ws)
                _hip.check(L.fgnn_linear_wgrad_multi(P(x), R, cin, n, (ctypes.c_void_p * n)(*[P(t) for t in gys]), cc,
                                                     (ctypes.c_void_p * n)(*[P(t) for t in gws]), (ctypes.c_void_p * n)(*[P(t) for t in gbs]),
                                                     P(ws), nb, _hip.stream_ptr()))
            else:
                for gy, gw, gb, c in zip(gys, gws, gbs, couts):
                    ws = torch.empty(int(L.fgnn_linear_wgrad_workspace_bytes(R, cin, c)) // 4, device=dev)
                    keep.append(ws)
                    S = (c // 64) * (cin // 64)          # one map alone: the b16 family, LDS-staged only when wide and long
                    kernel = _hip.invoke('fgnn_linear_wgrad_kernel', R, cin, c, _hip.BF16, x.data_ptr() & 15, gy.data_ptr() & 15).decode()
                    assert kernel in ('linear_wgrad_b16_kernel S=%d' % S,) + (('linear_wgrad_lds_kernel S=%d' % S,) if S >= 8 and R >= 2048 else ())
                    _hip.check(L.fgnn_linear_wgrad(P(x), P(gy), R, cin, c, _hip.BF16, P(gw), P(gb), P(ws), ws.numel() * 4, _hip.stream_ptr()))
        finally:
            L.fgnn_fold_defer(0)
        if deferred:
            assert L.fgnn_fold_pending() == n
            _hip.check(L.fgnn_fold_flush(_hip.stream_ptr()))
        assert L.fgnn_fold_pending() == 0
        torch.cuda.synchronize()
        return gws, gbs

    gws, gbs = run(True)
    for gy, gw, gb in zip(gys, gws, gbs):
        ref_w = gy.double().t() @ x.double()
        ref_b = gy.double().sum(0)
        assert float(((gw.double() - 1.0) - ref_w).abs().max()) <= 2e-5 * float(ref_w.abs().max()) + 1e-5
        assert float(((gb.double() - 2.0) - ref_b).abs().max()) <= 2e-5 * float(ref_b.abs().max()) + 1e-5
    gws2, gbs2 = run(True)
    assert all(torch.equal(a, b) for a, b in zip(gws + gbs, gws2 + gbs2))
    gws1, gbs1 = run(False)                      # map by map: other grids (row-waves per slice), so equal to f32 rounding, not to the bit
    for a, b in zip(gws + gbs, gws1 + gbs1):
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max())


def test_weight_gradients_of_several_maps_refuses_what_it_cannot_tile(dev):
    import ctypes
    from fgnn_amd import _hip
    L = _hip.lib()
    q = lambda cin, couts: int(L.fgnn_linear_wgrad_multi_workspace_bytes(4096, cin, len(couts), (ctypes.c_int32 * len(couts))(*couts)))
    assert q(256, (64, 256, 64)) == -1 and q(64, (32, 64)) == -1 and q(96, (64, 64)) == -1 and q(64, (64, 64, 64, 64)[:3]) > 0
    x = torch.zeros(4096, 256, device=dev, dtype=torch.bfloat16)
    gy = torch.zeros(4096, 256, device=dev, dtype=torch.bfloat16)
    gw = torch.zeros(256, 256, device=dev)
    ws = torch.zeros(1 << 20, device=dev)
    P = _hip._ptr
    rc = L.fgnn_linear_wgrad_multi(P(x), 4096, 256, 3, (ctypes.c_void_p * 3)(P(gy), P(gy), P(gy)), (ctypes.c_int32 * 3)(64, 256, 64),
                                   (ctypes.c_void_p * 3)(P(gw), P(gw), P(gw)), None, P(ws), ws.numel() * 4, _hip.stream_ptr())
    assert rc == _hip.EUNSUPPORTED
    # a map the b16 family takes, handed less workspace than its plan needs (more than the general kernel's): an error, no other kernel
    need = int(L.fgnn_linear_wgrad_workspace_bytes(4096, 256, 256))
    ws = torch.zeros(need // 4, device=dev)
    rc = L.fgnn_linear_wgrad(P(x), P(gy), 4096, 256, 256, _hip.BF16, P(gw), None, P(ws), need - 1024, _hip.stream_ptr())
    assert rc == -1 and b'workspace' in L.fgnn_last_error()


@pytest.mark.parametrize('cin,cout', [(64, 64), (64, 128), (128, 256), (256, 256), (256, 128), (128, 64)])
@pytest.mark.parametrize('N', [96, 48])
def test_iid_mapping_in_as_one_kernel(cin, cout, N, dev, monkeypatch):
    """`iid_mapping_in` (Conv2d 1x1 -> InstanceNorm2d -> ReLU, base_model.py:82-90) as ONE kernel (linear_instnorm_fwd_kernel) for
    bf16 states of 96 / 48 nodes: the kernel ran; output within bf16 rounding of the f32 torch chain on the same (rounded) inputs
    and of the staged two-kernel path; without a backward no pre-norm tensor is stored; with one, the gradients equal the staged
    path's (the same backward kernels on the same stored z) up to the rounding of z's statistics."""
    from fgnn_amd import ops
    from fgnn_amd.mpnn import blocks, iid_mapping_in
    g = torch.Generator().manual_seed(cin + cout + N)
    B = 37
    monkeypatch.setattr(blocks, '_IID_FUSE_MAX_CIN', 256)                     # (the dispatch keeps inputs wider than 128 staged: slower there)
    m = iid_mapping_in(cin, cout).to(dev)
    x = (torch.randn(B, N, 1, cin, generator=g) * 1.3 + 0.2).bfloat16().to(dev).permute(0, 3, 1, 2)
    gy = torch.randn(B, N, 1, cout, generator=g).bfloat16().to(dev).permute(0, 3, 1, 2)

    def run(fused, grad=True):
        monkeypatch.setattr(blocks, 'FUSE_IID_IN', fused)
        rec = []
        ops.TIMER = type('T', (), {'run': staticmethod(lambda sym, nb, nf, launch, use_note=True, **kw: (rec.append(sym), launch()))})()
        try:
            for q in m.parameters():
                q.grad = None
            xd = x.detach().requires_grad_(grad)
            with torch.autocast('cuda', dtype=torch.bfloat16), (contextlib.nullcontext() if grad else torch.no_grad()):
                y = m(xd)
            if grad:
                y.backward(gy)
        finally:
            ops.TIMER = None
        return (y.detach().float(), xd.grad.float() if grad else None, m.main[0].weight.grad.clone() if grad else None,
                m.main[0].bias.grad.clone() if grad else None, rec)

    f, s = run(True), run(False)
    assert 'linear_instnorm_fwd_kernel' in f[4] and 'instnorm_fwd_kernel' not in f[4], f[4]
    assert 'linear_instnorm_fwd_kernel' not in s[4] and 'instnorm_fwd_kernel' in s[4], s[4]
    # the f32 chain on the same bf16-rounded inputs and weights rounded as the kernels round them
    w = m.main[0].weight.detach().float().view(cout, cin).bfloat16().float()
    z = (x.float().permute(0, 2, 3, 1).reshape(B * N, cin) @ w.t() + m.main[0].bias.detach().float()).bfloat16().float()
    zr = z.view(B, N, cout).permute(0, 2, 1).unsqueeze(-1)
    ref = torch.relu(torch.nn.functional.instance_norm(zr, eps=1e-5))
    # (the staged path's wide maps come from the library GEMM, whose algorithm choice — and with it a bf16 ulp here and there, amplified by
    # the normalisation — is not the same in every process: 0.0080 against the usual 0.004 - 0.007 once in ~10 processes, round 6)
    assert H.rel_err(f[0], ref) <= 2.0 ** -7 and H.rel_err(s[0], ref) <= (2.0 ** -7 if cin * cout <= 8192 else 1.5 * 2.0 ** -7)
    assert H.rel_err(f[0], s[0]) <= 2.0 ** -7
    for a, b in zip(f[1:4], s[1:4]):
        # same backward kernels on the stored z.  Narrow maps: the staged z comes from the same MFMA arithmetic, bit for bit; wide
        # maps: from the library GEMM, one bf16 ulp away here and there — elements within rounding of the ReLU kink then take the
        # other branch in one of the two runs (an O(1) difference in THEIR gradient): compare in the mean there
        if cin * cout <= 8192:
            assert H.rel_err(a.float(), b.float()) <= 2.0 ** -9
        elif a.dim() > 1:                # (the bias gradient is sum_n dz = 0 in exact arithmetic: rounding noise on both sides)
            assert float((a.float() - b.float()).abs().mean()) <= 1e-2 * float(b.float().abs().mean())
    e = run(True, grad=False)
    assert 'linear_instnorm_fwd_kernel' in e[4] and torch.equal(e[0], f[0])
