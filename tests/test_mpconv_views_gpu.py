"""GPU: the message operator on strided, offset and batch-shared VIEWS of x, etype and nn_idx -- the layout rules of the six forward
and six backward families (their FGNN_REJECT lines and the ``return 0`` lines of the b16 / resident / ext plans).  The table, the
builders, the references and the bounds: tests/mpconv_view_cases.py (its contract is tests/test_mpconv_view_cases.py, CPU).

Every case runs its call twice, on the view and on a dense, 16-byte aligned clone of the same values, and asserts
  * the kernel ``fgnn_last_kernel`` reports, for both, template arguments included;
  * the same kernel on view and clone: every output bit for bit (loads do not change the arithmetic);
  * different kernels: the outputs within the family's bound of each other;
  * both against the CPU reference at that bound, so the file stands on its own: forward within the derived per-element bound of
    mpconv_b16_cases (bf16) or 1e-4 of the range (f32), the argmax under the near-tie rule; the gradients within 2^-6 of their range
    and 4 d per node / edge (bf16), 2^-7 (hyper-edge kinds), 1e-4 / 2e-4 (f32);
  * every byte of every base allocation, guard bands and inputs alike, unchanged after the call.
The statistics kinds run training-mode mp_conv_v2 on the view against the staged path (ops.STATS_EPILOGUE = False) on the clone:
output, running_mean, running_var, and the handed-off scale and shift.  No case picks its family through an environment switch.

What the cases found.  Two calls that raised on a legal view, both of one kind: a pointer-free query promised a kernel whose plan
then failed the call on a pointer.  (1) Training-mode mp_conv_v2 on a table-driven shape with x or etype off a 16-byte boundary:
fgnn_mpconv_forward_stats_partials announced the table-driven grid, fgnn_fwd_ws_plan rule 11 then failed the statistics call with
FGNN_EINVAL.  (2) The f32 synthetic-PGM backward with batch-shared edge types and x off a 16-byte boundary:
fgnn_mpconv_backward_reduces_getype said yes, fgnn_bwd_ext_plan then failed the reduced form.  ops now asks neither query for such
a view: the first call runs the plain forward and the BatchNorm's own pass (mpconv_fwd_b16_kernel<4, 0, 2, 2, 1, 6> then bn_stats on
the 64 -> 64 shape: output and running statistics bit-equal to the staged path), the second the generic backward and a batch sum.
(3) Views that fell through to kernels with other rounding points.  mpconv_fwd_ws, mpconv_fwd_b16 and mpconv_fwd_fanin round the
projections P to bf16; the resident, generic and identity-list fan-in kernels keep them in f32.  mpconv_fwd_b16 turned down a sample
stride that is no multiple of 8, a channel slice of wider rows and padded edge-type rows, and the fan-in kernels also a misaligned x,
although all of them read x with plain 16-byte global loads that need no alignment (mpconv_fwd_b16 had no pointer rule at all and
gives the same bits on an x two bytes off a boundary).  Such a view therefore ran the resident or generic kernel, or the
identity-list fan-in's ran mpconv_fwd_b16, and lay 1.03 - 1.39 of the derived bound from its dense clone (each alone within 0.94 of
it against the f64 reference), and in the training-mode call up to 1.16e-2 from the staged path where 2^-7 is asked: 42 cases.  The
two plans now take any row stride, sample stride and address of a channel-fastest x, and mpconv_fwd_b16 padded edge-type rows
(the kernels take the row strides from the descriptor): those views stay with the family of their dense call.

First measured on an MI355X (677 cases in about 10 s: table-driven kinds 312 = 126 forward + 60 backward + 126 statistics; b16 and
F8 93; hyper-edge fan-in 68, fan-out 36; ext 96; resident f32 36; generic 36; all pass, none above a second).  Forward: error at most 0.94 of the
derived bound (0.985 fan-out), 3e-3 of the f32 bound, the argmax gap at most 0.09 of the near-tie slack; mpconv_fwd_b16 against
mpconv_fwd_ws on the same values: equal in every bit at B = 5, at most 0.60 of the bound apart at B = 300.  Backward: z and the
gradients at most 1.02e-2 of their range in bf16 (bound 1.56e-2), 9.2e-6 in f32; worst node 1.59e-2 against 4 d = 1.81e-2 (ws6 at
B = 300), worst edge 1.91e-2 against 2.48e-2 (ws6x2); 113 of 188 runs bit-equal to the clone.  No byte of any base allocation
changed."""
import pytest
import torch

import helpers as H
import mpconv_b16_cases as C
import mpconv_sg_cases as S
import mpconv_view_cases as V

pytestmark = pytest.mark.gpu

TABLE = V.cases()
BY_MODE = {m: [c for c in TABLE if c[3] == m] for m in ('fwd', 'bwd', 'stats')}


@pytest.fixture(scope='module')
def shared():
    """One problem per (kind, B) and one forward reference per (kind, B, batch-expanded operands): kept while the table stays with
    that kind and batch size."""
    made = {}

    def get(kind, B, geometry):
        if made.get('at') != (kind, B):
            made.clear()
            made['at'], made['problem'] = (kind, B), V.problem(kind, B)
        q = V.values_for(made['problem'], geometry)
        variant = tuple(n for n in ('x', 'et', 'idx') if V.GEOMETRIES[geometry].get(n, {}).get('expand'))
        if variant not in made:
            made[variant] = V.forward_reference(q, V.dense_clone(q, torch.device('cpu')))
        return q, made[variant]
    return get


def _same_kernel(kern, want):
    return kern.startswith(want) if want.endswith(', ') else kern == want


def _clone_kernel(kind, geometry, which):
    """The dense clone runs the kind's control kernel; B written-out copies of one table are recognised as one (ops.shared_graph_view)."""
    return V.expect(kind, geometry if geometry == 'idx_expand' else 'dense')[which]


def _forward_errors(q, ref, z, am):
    dtype = V.KINDS[q['kind']][0]
    ratio = float(((z.double() - ref['z']).abs() / ref['bound']).max())
    assert bool(torch.isfinite(z).all()) and 0 <= int(am.min()) and int(am.max()) < ref['E'].shape[2]
    return ratio, S.rel_err(z, ref['z']), V.tie_gap(am, ref, dtype)


@pytest.mark.parametrize('case', BY_MODE['fwd'], ids=[V.case_id(c) for c in BY_MODE['fwd']])
def test_forward_on_a_view(case, shared, dev):
    kind, B, geometry, _ = case
    q, ref = shared(kind, B, geometry)
    dtype = V.KINDS[kind][0]
    o, c = V.operands(q, geometry, dev), V.dense_clone(q, dev)
    snap = V.snapshot(o)
    z, am, kern = V.device_forward(q, o)
    z2, am2, kern2 = V.device_forward(q, c)
    e = V.expect(kind, geometry)
    ev, ec = _forward_errors(q, ref, z, am), _forward_errors(q, ref, z2, am2)
    apart = float(((z.double() - z2.double()).abs() / ref['bound']).max())
    print('%s: view %s (rules %s), clone %s; error / bound %.3f | %.3f, of the range %.2e | %.2e, argmax gap / slack %.3f | %.3f, '
          'view - clone / bound %.3f' % (V.case_id(case), kern, ', '.join(e['fwd_rules']) or '-', kern2, ev[0], ec[0], ev[1], ec[1], ev[2],
                                         ec[2], apart))
    assert _same_kernel(kern, e['fwd']), (kern, e['fwd'])
    assert _same_kernel(kern2, _clone_kernel(kind, geometry, 'fwd')), kern2
    for ratio, err, gap in (ev, ec):
        assert ratio <= 1.0 and gap <= 1.0 and (dtype != V.BF16 or err <= C.TOL), (ratio, err, gap)
    assert V.unchanged(o, snap)
    if kern == kern2:
        assert torch.equal(z, z2) and torch.equal(am, am2)
    else:
        assert apart <= 1.0, 'view and clone %.3f of the bound apart (%s | %s)' % (apart, kern, kern2)


def _range_err(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-20))


def _backward_errors(q, o_cpu, out):
    """One run against autograd through its own routing: the errors of z, gx, getype, gW, gbias (getype None where the kind takes
    none), and the worst node / edge over that row's own range where the kind has the yardstick."""
    kind = q['kind']
    dtype, shape, _, group = V.KINDS[kind][:4]
    z, am, gx, get, gW, gb = out[:6]
    ref = V.backward_reference(q, o_cpu, am)
    rget = ref[2] if get is None or get.shape[0] == ref[2].shape[0] else ref[2].sum(0, keepdim=True)
    err = S.rel_err if dtype == V.BF16 else _range_err
    errs = [err(z, ref[0]), err(gx, ref[1]), None if get is None else err(get, rget), err(gW, ref[3]), err(gb, ref[4])]
    assert bool(torch.isfinite(gx).all())
    node = edge = None
    if kind in V.D:
        node, stray = S.per_row_error(gx, ref[1], (0, 2))
        assert stray == 0
        if get.shape[0] == ref[2].shape[0]:
            edge, stray = S.per_row_error(get, rget, (0, 3))
            assert stray == 0
    return errs, node, edge


def _backward_bounds(kind):
    dtype, _, _, group = V.KINDS[kind][:4]
    if dtype == V.BF16:
        g = V.HYPER_TOL if group in ('fanin', 'fanout') else S.TOL
        return [S.TOL, g, S.TOL, g, g]
    return [V.F32_TOL.get(group, 1e-4)] * 5


@pytest.mark.parametrize('case', BY_MODE['bwd'], ids=[V.case_id(c) for c in BY_MODE['bwd']])
def test_backward_on_a_view(case, shared, dev):
    kind, B, geometry, _ = case
    q, _ = shared(kind, B, geometry)
    cpu = torch.device('cpu')
    o, c = V.operands(q, geometry, dev), V.dense_clone(q, dev)
    snap = V.snapshot(o)
    a, b = V.device_backward(q, o), V.device_backward(q, c)
    e = V.expect(kind, geometry)
    o_cpu = V.dense_clone(q, cpu)
    (ea, na, da), (eb, nb, db) = _backward_errors(q, o_cpu, a), _backward_errors(q, o_cpu, b)
    fmt = lambda v: ' '.join('-' if x is None else '%.2e' % x for x in v)
    print('%s: view %s then %s (rules %s), clone %s then %s; z gx getype gW gbias %s | %s; worst node %s | %s, worst edge %s | %s' % (
        V.case_id(case), a[6], a[7], ', '.join(e['bwd_rules']) or '-', b[6], b[7], fmt(ea), fmt(eb), fmt([na]), fmt([nb]), fmt([da]), fmt([db])))
    assert _same_kernel(a[6], e['fwd']) and _same_kernel(a[7], e['bwd']), (a[6], a[7], e)
    assert _same_kernel(b[6], _clone_kernel(kind, geometry, 'fwd')) and _same_kernel(b[7], _clone_kernel(kind, geometry, 'bwd')), b[6:]
    et_shared = o.et_leaf.shape[0] == 1 and B > 1
    if V.KINDS[kind][7]:
        assert a[3].shape[0] == (1 if et_shared else B)          # batch-expanded edge types: the gradient summed over the batch
    if a[6] == b[6] and a[7] == b[7]:
        for u, v in zip(a[:6], b[:6]):
            if u is not None and u.shape == v.shape:
                assert torch.equal(u, v)
    bounds = _backward_bounds(kind)
    for errs, node, edge in ((ea, na, da), (eb, nb, db)):
        for got, bound in zip(errs, bounds):
            assert got is None or got <= bound, (errs, bounds)
        if node is not None:
            assert node <= 4 * V.D[kind][0], (node, V.D[kind])
        if edge is not None:
            assert edge <= 4 * V.D[kind][1], (edge, V.D[kind])
    assert V.unchanged(o, snap)


def _module(kind, dev):
    from fgnn_amd.mpnn import mp_conv_type, mp_conv_v2
    nin, nou, net = V.KINDS[kind][1][:3]
    torch.manual_seed(7)
    m = mp_conv_v2(nin, nou, net, extension=mp_conv_type.NO_EXTENSION, aggregtor='max').to(dev).train()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        m.bn.weight.copy_((torch.rand(nou, generator=g) + 0.5).to(dev))
        m.bn.bias.copy_((torch.randn(nou, generator=g) * 0.3).to(dev))
    return m


def _train_forward(kind, o, dev, epilogue):
    """Training-mode mp_conv_v2 on the operands: (y, running_mean, running_var, the kernels that ran)."""
    from fgnn_amd import ops
    m = _module(kind, dev)
    ops.STATS_EPILOGUE = epilogue
    ops.TIMER = ops.KernelTimer()
    try:
        y = m(o.x, o.idx, o.et)
        names = set(ops.TIMER.summary())
    finally:
        ops.STATS_EPILOGUE = True
        ops.TIMER = None
    return y.detach().float().cpu(), m.bn.running_mean.cpu(), m.bn.running_var.cpu(), names


@pytest.mark.parametrize('case', BY_MODE['stats'], ids=[V.case_id(c) for c in BY_MODE['stats']])
def test_training_mode_forward_on_a_view(case, shared, dev):
    """The call that used to raise on a misaligned view.  The reference is the staged path on the dense clone."""
    from fgnn_amd import _hip, ops
    from fgnn_amd.mpnn.pointwise import BnHandoff
    kind, B, geometry, _ = case
    q, _ = shared(kind, B, geometry)
    nou, net = V.KINDS[kind][1][1:3]
    o, c = V.operands(q, geometry, dev), V.dense_clone(q, dev)
    snap = V.snapshot(o)
    want, epilogue = V.expect_stats(kind, geometry)
    y, rm, rv, names = _train_forward(kind, o, dev, True)
    y2, rm2, rv2, names2 = _train_forward(kind, c, dev, False)
    e_y, e_m, e_v = H.rel_err(y, y2), H.rel_err(rm, rm2), H.rel_err(rv, rv2)
    # the hand-off itself: the statistics the operator's launch leaves for the BatchNorm behind it
    m = _module(kind, dev)
    h = BnHandoff.of(m.bn)
    ops.mpconv_forward_raw(o.x, o.idx, o.et, m.filters, m.bias, nou, net, 0, _hip.AGG_MAX, bn=h, want_argmax=True)
    e_s = e_t = None
    if h.stats is not None:
        z2, _ = ops.mpconv_forward_raw(c.x, c.idx, c.et, m.filters, m.bias, nou, net, 0, _hip.AGG_MAX)
        zz = z2.double()
        mean, var = zz.mean((0, 2, 3)), zz.var((0, 2, 3), unbiased=False)
        scale = m.bn.weight.detach().double() / (var + m.bn.eps).sqrt()
        e_s, e_t = H.rel_err(h.stats[2], scale), H.rel_err(h.stats[3], m.bn.bias.detach().double() - mean * scale)
    print('%s: %s, %s; y %.2e (%.2e) running_mean %.2e (1e-5) running_var %.2e (1e-4) scale %s shift %s (1e-4)' % (
        V.case_id(case), sorted(n for n in names if n.startswith('mpconv_fwd')), 'epilogue' if h.stats is not None else 'bn_stats pass',
        e_y, V.STATS_TOL['y'], e_m, e_v, e_s, e_t))
    assert any(_same_kernel(n, want) for n in names), (names, want)
    assert any(n.startswith('bn_stats') for n in names) == (not epilogue and bool(_hip.lib().fgnn_bn_supported(B * q['gz'].shape[1], nou, _hip.dtype_code(o.x)))), names
    assert (h.stats is not None) == epilogue
    assert any(n.startswith('bn_stats') for n in names2) or not _hip.lib().fgnn_bn_supported(B * q['gz'].shape[1], nou, _hip.dtype_code(o.x))
    if epilogue:
        assert e_s <= V.STATS_TOL['var'] and e_t <= V.STATS_TOL['var']
    assert V.unchanged(o, snap)
    assert e_y <= V.STATS_TOL['y'] and e_m <= V.STATS_TOL['mean'] and e_v <= V.STATS_TOL['var'], (e_y, e_m, e_v)
