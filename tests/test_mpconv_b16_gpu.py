"""GPU: the catch-all bf16 operator kernels (csrc/mpconv_fwd_b16.hip, csrc/mpconv_bwd_b16.hip) on the calls the table-driven and
hyper-edge families turn down, away from the LDPC shapes the rest of the suite runs them at: the neighbour-list split over waves (JP > 1:
partials through LDS, empty and short parts, all three cross-wave combines, the region reused across column passes), the mean
aggregator, plain [B, net, M, k] edge types, partly filled channel blocks and slab sets, more than one block of ids per part, the staging
limits met exactly, a workgroup that takes a second sample, the statistics epilogue below 64 channels, and the backward up to k = 255.
Cases, generator, references and bounds: tests/mpconv_b16_cases.py (its contract is tests/test_mpconv_b16_cases.py, CPU).  Every case
asserts the kernel through ``fgnn_last_kernel``, template arguments included, so a dispatch change cannot quietly move it elsewhere.

Bounds.  Forward: every element within its own derived bound (the case module's docstring), and the project's 2^-6 of the output range
as a ceiling; for max, the argmax names a neighbour whose f64 message is within b_j + b_j* of the true maximum j*'s, and in the tied runs (every
destination lists its slot-0 node again in slot k - 1, bit-equal messages in different parts of the split) never slot k - 1.  Backward:
2^-6 of each gradient's range against torch autograd through the kernel's own argmax; per node of gx and per edge of getype 4 d, d the
case's CPU-measured rounding-model error (``C.D``); gx of a node nobody lists zero in every bit.  The figures are printed (-s).

What these cases found: no wrong value.  First measured on an MI355X, every run on the kernel its case names: forward error at most 0.937
of the derived bound (F8 at B = 1029; 0.89 among the B = 6 runs, F7) and 4.4e-03 of the output range, argmax gap at most 0.62 of
b_j + b_j*, none of the tied runs' outputs names the last slot.  Backward: z and the gradients at most 4.4e-03 of their range; on
mpconv_bwd_b16 the worst node and edge are the CPU model's own d to four digits (5.85e-03 F2, 1.87e-02 F13), on the generic kernel (F8)
7.39e-03 / 9.32e-03 against 4 d = 1.82e-02 / 2.36e-02, on the resident one below d.  F15 and E3 (M k net 1600 and 2040) take
mpconv_fwd_res_kernel<bf16_t, 4, 0, 16, 2, 1> in front of mpconv_bwd_b16_kernel<2, 2>; F9, E2 and the plain-layout runs take
mpconv_bwd_res_kernel, which stands before the generic kernel in the dispatch table and takes bf16 operands."""
import pytest
import torch

import helpers as H
import mpconv_b16_cases as C
import mpconv_sg_cases as S

pytestmark = pytest.mark.gpu

FORWARD_RUNS = [(name, agg, layout) for name, shape, _, _ in C.FORWARD for agg in C.AGGS
                for layout in (('fastest', 'plain') if shape[2] == 4 else ('fastest',))]     # net = 1: the two layouts coincide


@pytest.fixture(scope='module')
def reference():
    """One problem and one f64 reference per (case, B, tied, shared, aggregator), shared by the runs that read it."""
    made = {}

    def get(name, agg, B=C.B_SMALL, shared=False):
        tied = agg == 'max' and name in C.TIED
        if (name, agg, B, shared) not in made:
            q = made.setdefault((name, tied, B, shared), C.problem(name, B, tied=tied, shared=shared))
            made[name, agg, B, shared] = (q, C.forward_reference(q, agg))
        return made[name, agg, B, shared]
    return get


def check_forward(q, ref, agg, z, am, kern, what):
    nin, nou, net, N, M, k = q['shape']
    want = C.forward_kernel(q['shape'], agg)
    ratio, err = C.bound_ratio(z, ref), S.rel_err(z, ref['z'])
    line = '%s %s: %s, error / derived bound %.3f, %.2e of the range (ceiling %.2e)' % (q['name'], what, kern, ratio, err, C.TOL)
    if agg == 'max':
        assert am is not None and 0 <= int(am.min()) and int(am.max()) < k, line
        gap, _ = C.argmax_gap_ratio(am, ref)
        line += ', argmax gap / (b_j + b_j*) %.3f' % gap
        if q['tied']:
            last = int((am == k - 1).sum())
            line += ', %d of %d outputs name the tied last slot' % (last, am.numel())
    print(line)
    assert kern.startswith(want) and (want.endswith(', ') or kern == want), (kern, want)
    assert bool(torch.isfinite(z).all()) and ratio <= 1.0 and err <= C.TOL, line
    if agg == 'max':
        assert gap <= 1.0, line
        if q['tied']:
            assert last == 0, line                          # first occurrence, within a wave and in the cross-wave combine


@pytest.mark.parametrize('name,agg,layout', FORWARD_RUNS, ids=['-'.join(r) for r in FORWARD_RUNS])
def test_forward_within_the_derived_bound(name, agg, layout, reference, dev):
    q, ref = reference(name, agg)
    z, am, kern = C.device_forward(q, agg, dev, layout)
    check_forward(q, ref, agg, z, am, kern, '%s %s' % (agg, layout))


@pytest.mark.parametrize('name', C.LARGE_BATCH)
def test_forward_when_a_workgroup_takes_a_second_sample(name, reference, dev):
    """B = 1029 on a small-LDS shape: the grid is 1024, so five workgroups commit a prefetched second sample (and, for F1, reuse the
    partials' region across samples)."""
    assert C.plan_model(C.SHAPE[name])['grid_cap'] < C.B_LARGE
    q, ref = reference(name, 'max', B=C.B_LARGE)
    z, am, kern = C.device_forward(q, 'max', dev)
    check_forward(q, ref, 'max', z, am, kern, 'max B=%d' % C.B_LARGE)
    tail = {n: v[1024:] for n, v in ref.items()}            # the second samples on their own
    assert C.bound_ratio(z[1024:], tail) <= 1.0 and C.argmax_gap_ratio(am[1024:], tail)[0] <= 1.0


@pytest.mark.parametrize('name', C.SHARED_TABLE)
@pytest.mark.parametrize('agg', C.AGGS)
def test_forward_with_a_batch_shared_table(name, agg, reference, dev):
    q, ref = reference(name, agg, shared=True)
    assert q['idx'].shape[0] == 1
    z, am, kern = C.device_forward(q, agg, dev)
    check_forward(q, ref, agg, z, am, kern, '%s shared table' % agg)


@pytest.mark.parametrize('name', C.AFFINE)
@pytest.mark.parametrize('agg', C.AGGS)
def test_forward_affine_and_relu_epilogue(name, agg, dev):
    """bias, post_scale (both signs), post_shift and ReLU behind the split path's combine: the same affine on the reference, the bound's
    first term scaled by |post_scale|."""
    q = C.problem(name)
    aff = C.affine_of(q)
    ref = C.forward_reference(q, agg, aff, True)
    z, _, kern = C.device_forward(q, agg, dev, affine=aff, relu=True)
    ratio, err = C.bound_ratio(z, ref), S.rel_err(z, ref['z'])
    print('%s %s affine + ReLU: %s, error / derived bound %.3f, %.2e of the range' % (name, agg, kern, ratio, err))
    assert kern == C.forward_kernel(q['shape'], agg), kern
    assert float(z.min()) == 0.0 and ratio <= 1.0 and err <= C.TOL


@pytest.mark.parametrize('name', C.STATISTICS)
def test_statistics_epilogue_below_64_channels(name, dev):
    """Training-mode mp_conv_v2 at nou = 48 and 20: the forward's epilogue leaves the BatchNorm's batch statistics (lanes >= nou stay
    out of them).  running_mean / running_var are torch's momentum blend of the f64 mean and unbiased variance of the stored z -- the
    same kernel run without the epilogue -- and the module's output is that z normalised; no bn_stats pass."""
    from fgnn_amd import _hip, ops
    from fgnn_amd.mpnn import mp_conv_type, mp_conv_v2
    q = C.problem(name, B=37)
    nin, nou, net, N, M, k = q['shape']
    assert C.plan_model(q['shape'], stats=True) is not None
    xd, idxd, etd = C._operands(q, dev, 'fastest')
    torch.manual_seed(7)
    m = mp_conv_v2(nin, nou, net, extension=mp_conv_type.NO_EXTENSION, aggregtor='max').to(dev).train()
    ops.TIMER = ops.KernelTimer()
    try:
        y = m(xd, idxd, etd)
        names = set(ops.TIMER.summary())
    finally:
        ops.TIMER = None
    assert C.forward_kernel(q['shape'], 'max') in names and not any(n.startswith('bn_stats') for n in names), names
    z, _ = ops.mpconv_forward_raw(xd, idxd, etd, m.filters, m.bias, nou, net, 0, _hip.AGG_MAX)
    assert _hip.lib().fgnn_last_kernel().decode() == C.forward_kernel(q['shape'], 'max')
    zz = z.double().cpu()
    mean, var = zz.mean((0, 2, 3)), zz.var((0, 2, 3), unbiased=True)
    mom = m.bn.momentum
    e_mean = H.rel_err(m.bn.running_mean.cpu().double(), mom * mean)
    e_var = H.rel_err(m.bn.running_var.cpu().double(), (1 - mom) + mom * var)
    # what the module normalised IS this z.  The fused BatchNorm + ReLU kernel takes 8 bf16 channels per lane and a power-of-two number
    # of such lanes per row, so at 48 and 20 channels the module hands z to torch's own bf16 batch_norm: the output must be that
    # function of the plain launch's z, bit for bit.  (Against an f64 normalisation torch's bf16 kernel itself is 4.0e-3 / 3.1e-2 of
    # the range off at 48 / 20 channels on an MI355X, its f32 one 3e-7 on the same z; that figure is torch's, printed for the record.)
    assert not _hip.lib().fgnn_bn_supported(q['B'] * M, nou, _hip.dtype_code(z))
    own = torch.relu(torch.nn.functional.batch_norm(z, None, None, m.bn.weight, m.bn.bias, True, 0.0, m.bn.eps))
    norm = torch.relu((zz - mean[None, :, None, None]) / (zz.var((0, 2, 3), unbiased=False) + m.bn.eps).sqrt()[None, :, None, None])
    print('%s statistics epilogue: running_mean %.2e (1e-5), running_var %.2e (1e-4); torch\'s bf16 batch_norm of z against f64 %.2e' % (
        name, e_mean, e_var, H.rel_err(own.detach().double().cpu(), norm)))
    assert e_mean <= 1e-5 and e_var <= 1e-4
    assert y.stride() == own.stride() and torch.equal(y.detach(), own.detach())


def check_backward(name, layout, want, dev):
    q = C.problem(name)
    nin, nou, net, N, M, k = q['shape']
    z, am, gx, get, gW, gb, fwd, bwd = C.device_backward(q, 'max', dev, layout)
    ref = S.routed_reference(q['x'], q['idx'], q['et'], q['W'], q['bias'], q['gz'], am)
    errs = [S.rel_err(a, b) for a, b in zip((z, gx, get, gW, gb), ref)]
    node, stray_n = S.per_row_error(gx, ref[1], (0, 2))
    edge, stray_e = S.per_row_error(get, ref[2], (0, 3))
    empty = C.empty_nodes(q['idx'], q['B'], N)
    d_node, d_edge = C.D[name]
    print('%s %s: %s then %s, errors z %.2e gx %.2e getype %.2e gW %.2e gbias %.2e (bound %.2e), worst node %.4e (4 d = %.4e), worst '
          'edge %.4e (4 d = %.4e), %d empty node rows' % (name, layout, fwd, bwd, *errs, C.TOL, node, 4 * d_node, edge, 4 * d_edge,
                                                        int(empty.sum())))
    assert fwd.startswith(C.forward_kernel(q['shape'], 'max')), fwd
    assert bwd.startswith(want), (bwd, want)
    if layout == 'fastest':
        assert ('mpconv_bwd_b16' in bwd) == (C.backward_family(q['shape']) == 'mpconv_bwd_b16'), bwd
    assert int(am.max()) < k and max(errs) <= C.TOL, errs
    assert bool(torch.isfinite(gx).all()) and stray_n == 0 and stray_e == 0
    assert int((gx[empty].view(torch.int32) != 0).sum()) == 0                  # every bit: -0.0 counts
    assert node <= 4 * d_node and edge <= 4 * d_edge, (node, edge)


@pytest.mark.parametrize('name,want', C.BACKWARD, ids=[n for n, _ in C.BACKWARD])
def test_backward_vs_routed_reference(name, want, dev):
    """Every max, 4-edge-type case and the three at rule 7's edges (N = 9 | 8, k = 255) through ops.mpconv and backward.  F15 and
    E3 pair a forward of another family (M k net beyond mpconv_fwd_b16's staging registers) with mpconv_bwd_b16."""
    check_backward(name, 'fastest', want, dev)


@pytest.mark.parametrize('name,want', C.BACKWARD_PLAIN, ids=[n for n, _ in C.BACKWARD_PLAIN])
def test_backward_with_plain_edge_types_leaves_the_family(name, want, dev):
    check_backward(name, 'plain', want, dev)


@pytest.mark.parametrize('name', C.BACKWARD_ORACLE)
@pytest.mark.parametrize('agg', ['softmax', 'mean'])
def test_softmax_and_mean_backward_vs_oracle_autograd(name, agg, dev):
    """The generic backward behind mpconv_fwd_b16's softmax and mean, channel-fastest bf16 operands, at these widths."""
    q = C.problem(name)
    out = C.device_backward(q, agg, dev)
    ref = C.oracle_autograd(q, agg)
    errs = [S.rel_err(a, b) for a, b in zip(out[:1] + out[2:6], ref)]
    print('%s %s: %s then %s, errors z %.2e gx %.2e getype %.2e gW %.2e gbias %.2e (bound %.2e)' % (name, agg, out[6], out[7], *errs, C.TOL))
    assert out[6] == C.forward_kernel(q['shape'], agg) and out[7].startswith('mpconv_bwd_kernel<bf16_t, %d, ' % q['shape'][2]), out[6:]
    assert max(errs) <= C.TOL, errs
