"""CPU contract of tests/mpconv_view_cases.py, the case table of tests/test_mpconv_views_gpu.py: every builder produces the geometry
its name claims (pointer alignment, strides, guard bands), the references give the same bits on a view as on its dense clone, the
table names a kernel for every case and a case for every layout rule of the twelve plans, and the per-node / per-edge yardstick the
backward cases use is the rounding model's own error."""
import pytest
import torch

import mpconv_b16_cases as C
import mpconv_sg_cases as S
import mpconv_view_cases as V

CPU = torch.device('cpu')
PAIRS = sorted({(kind, geometry) for kind, _, geometry, _ in V.cases()})


@pytest.fixture(scope='module')
def problems():
    made = {}
    return lambda kind: made.setdefault(kind, V.problem(kind, V.B_SMALL))


def _item(t):
    return t.element_size()


@pytest.mark.parametrize('kind,geometry', PAIRS, ids=['%s-%s' % p for p in PAIRS])
def test_builders_produce_the_named_geometry(kind, geometry, problems):
    q = V.values_for(problems(kind), geometry)
    o = V.operands(q, geometry, CPU)
    spec, B = V.GEOMETRIES[geometry], q['B']
    nin, nou, net, N, M, k = V.KINDS[kind][1]
    sh_idx, sh_et = V.KINDS[kind][5:7]
    assert o.x.shape == (B, nin, N, 1) and o.idx.shape == (B, M, k) and o.et.shape == (B, net, M, k)
    # every operand lies inside its base with the guard bands in place, and the bands hold the pattern
    for name, view in (('x', o.x), ('idx', o.idx), ('et', o.et)):
        base = o.bases[name]
        front, behind = V.guard_band(view, base)
        assert front >= V.SLACK and behind >= V.SLACK, (name, front, behind)
        as_int, bits = V.PATTERN[base.dtype]
        assert bool((base[:front].view(as_int) == bits).all()) and bool((base[base.numel() - behind:].view(as_int) == bits).all())
        assert base.data_ptr() % 16 == 0
    # x
    sx = spec.get('x', {})
    want_off = sx.get('off_el', 0) * _item(o.x) + (max(sx['off'], _item(o.x)) if 'off' in sx else 0)
    assert o.x.data_ptr() % 16 == want_off % 16 and (want_off == 0 or o.x.data_ptr() % 16 != 0)
    sn = nin + sx.get('sn_pad', 0)
    assert o.x.stride(1) == 1 and (N == 1 or o.x.stride(2) == sn)
    want_sb = 0 if sx.get('expand') else (N * sn + sx.get('sb_pad', 0)) * sx.get('every', 1)
    assert o.x.stride(0) == want_sb
    if sx.get('every'):
        assert o.x.stride(0) == 2 * N * nin
    # etype: edge-type fastest
    se = spec.get('et', {})
    want_off = max(se['off'], _item(o.et)) if 'off' in se else 0
    assert o.et.data_ptr() % 16 == want_off % 16 and (want_off == 0 or o.et.data_ptr() % 16 != 0)
    sm = (k + se.get('row_pad', 0)) * net
    assert o.et.stride(1) == 1 and (k == 1 or o.et.stride(3) == net) and (M == 1 or o.et.stride(2) == sm)
    shared = se.get('expand') or (sh_et and 'sb_pad' not in se)
    assert o.et.stride(0) == (0 if shared else M * sm + se.get('sb_pad', 0))
    assert o.et_leaf.shape[0] == (1 if shared else B)
    # nn_idx
    si = spec.get('idx', {})
    ck = k + si.get('col_pad', 0)
    assert (k == 1 or o.idx.stride(2) == 1) and (M == 1 or o.idx.stride(1) == ck)
    shared = (sh_idx and not si.get('copies')) or si.get('expand')
    assert o.idx.stride(0) == (0 if shared else (M + 2 * si.get('row_off', 0)) * ck)
    assert (o.idx.data_ptr() - o.bases['idx'].data_ptr()) == 8 * (V.SLACK + si.get('row_off', 0) * ck)
    if si.get('copies'):
        assert bool((o.idx == o.idx[:1]).all())
    # the values are the problem's, and the dense clone holds the same in the kind's own form
    c = V.dense_clone(q, CPU)
    for a, b in ((o.x, c.x), (o.idx, c.idx), (o.et, c.et)):
        assert torch.equal(a, b)
    assert c.x.stride() == (N * nin, 1, nin, nin) and c.idx.stride(0) == (0 if sh_idx else M * k) and c.et.stride(0) == (0 if sh_et else M * k * net)


@pytest.mark.parametrize('kind,geometry', PAIRS, ids=['%s-%s' % p for p in PAIRS])
def test_references_do_not_see_the_layout(kind, geometry, problems):
    """Bit-identical on a view and on its dense clone: forward and (where the case has one) backward."""
    q = V.values_for(problems(kind), geometry)
    o, c = V.operands(q, geometry, CPU), V.dense_clone(q, CPU)
    snap = V.snapshot(o)
    ro, rc = V.forward_reference(q, o), V.forward_reference(q, c)
    for n in ('z', 'bound', 'E'):
        assert torch.equal(ro[n], rc[n]), n
    assert bool(torch.isfinite(ro['z']).all()) and float(ro['bound'].min()) > 0
    if V.expect(kind, geometry)['bwd'] is not None:
        am = S.first_argmax(ro['E'])
        assert V.tie_gap(am, ro, V.KINDS[kind][0]) == 0.0
        threads = torch.get_num_threads()
        torch.set_num_threads(1)                # (autograd's scatter-adds run in one fixed order: the same bits twice)
        try:
            for a, b in zip(V.backward_reference(q, o, am), V.backward_reference(q, c, am)):
                assert torch.equal(a, b)
        finally:
            torch.set_num_threads(threads)
    assert V.unchanged(o, snap)


def test_every_case_names_its_kernels():
    table = V.cases()
    assert len(set(table)) == len(table)
    for kind, B, geometry, mode in table:
        e = V.expect(kind, geometry)
        dense = V.expect(kind, 'dense')
        assert e['fwd'].startswith('mpconv_fwd_') and (mode != 'bwd' or e['bwd'].startswith('mpconv_bwd_')), (kind, geometry)
        # a case that leaves the control's family says which rule sent it away, and only such a case does
        # (but: the per-sample kind's dense control names the rule that keeps it from the table-driven family, a batch-shared
        # table lifts that rule, and the hyper-edge backward's "packed" rule picks accesses, not a kernel)
        if geometry not in ('dense', 'idx_expand'):
            assert bool(e['fwd_rules']) == (e['fwd'] != dense['fwd']), (kind, geometry, e)
            if e['bwd'] is not None and 'hyper-edge backward packed' not in e['bwd_rules']:
                assert bool(e['bwd_rules']) == (e['bwd'] != dense['bwd']), (kind, geometry, e)
        for r in e['fwd_rules'] + e['bwd_rules']:
            assert r in V.RULES, r
        if mode == 'stats':
            name, epilogue = V.expect_stats(kind, geometry)
            assert name.startswith('mpconv_fwd_') and (epilogue or geometry != 'dense')
    # every kind has its dense control, the B = 300 runs exist, a backward only where Python hands the view on
    for kind in V.KINDS:
        modes = {(B, m) for k2, B, g, m in table if k2 == kind and g == 'dense'}
        assert ((V.B_SMALL, 'stats') in modes) == (kind in V.STATS_KINDS)
        assert ((V.B_LARGE, 'fwd') in modes) == (kind in V.LARGE_FWD) and ((V.B_LARGE, 'bwd') in modes) == (kind in V.LARGE_BWD)
    for kind, B, geometry, mode in table:
        if mode == 'bwd':
            sx = V.GEOMETRIES[geometry].get('x', {})
            assert not (set(sx) - {'off', 'off_el'}), (kind, geometry)
    # the b16 model of the case module agrees that these shapes are mpconv_fwd_b16's
    for kind in ('ws6', 'ws3k', 'ws6x2', 'b16', 'fanin', 'F8'):
        assert C.plan_model(V.KINDS[kind][1]) is not None
    assert C.plan_model(V.KINDS['F8'][1], stats=True) is not None and C.plan_model(V.KINDS['ws6'][1], stats=True) is not None
    assert C.plan_model(V.KINDS['ws6x2'][1], stats=True) is None


def test_every_layout_rule_is_named_by_a_case():
    assert len(set(V.RULES)) == len(V.RULES)
    named = set()
    for kind, _, geometry, mode in V.cases():
        e = V.expect(kind, geometry)
        named.update(e['fwd_rules'])
        if mode == 'bwd':
            named.update(e['bwd_rules'])
    exempt = dict(V.OUT_OF_REACH, **V.OTHER_LAYOUT)
    assert len(exempt) == len(V.OUT_OF_REACH) + len(V.OTHER_LAYOUT) and not (set(exempt) - set(V.RULES)) and not (named & set(exempt))
    missing = [r for r in V.RULES if r not in named and r not in exempt]
    assert not missing, missing


def rounding_model_error(kind):
    q = V.problem(kind, V.B_SMALL)
    nou = V.KINDS[kind][1][1]
    x, idx, et, W, bias, gz = q['x'], q['idx'], q['et'], q['W'], q['bias'], q['gz']
    _, E = S.messages(x.float(), idx, et.float(), W, nou)
    sel = S.first_argmax(E)
    ref = S.routed_reference(x, idx, et, W, bias, gz, sel)
    plain = S.routed_by_hand(x, idx, et, W, gz, sel, rounded=False)
    for u, v in zip(plain, ref[1:]):
        assert S.rel_err(u, v) <= 1e-5
    gx, get, _, _ = S.routed_by_hand(x, idx, et, W, gz, sel, rounded=True)
    node, stray_n = S.per_row_error(gx, ref[1], (0, 2))
    edge, stray_e = S.per_row_error(get, ref[2], (0, 3))
    assert stray_n == 0 and stray_e == 0
    return node, edge


@pytest.mark.parametrize('kind', sorted(V.D))
def test_rounding_model_error(kind):
    d_node, d_edge = rounding_model_error(kind)
    print('%-6s d_node %.4e  d_edge %.4e  (recorded: %.4e, %.4e)' % (kind, d_node, d_edge, *V.D[kind]))
    assert 0.98 * V.D[kind][0] <= d_node <= V.D[kind][0] and 0.98 * V.D[kind][1] <= d_edge <= V.D[kind][1]
