"""CPU: the contract of tests/mpconv_b16_cases.py, which tests/test_mpconv_b16_gpu.py relies on.  Every forward case's rounding model
(P and the output rounded to bf16, everything else f64) stays within the derived per-element bound; the per-node / per-edge yardstick
of the backward cases is measured here (run with -s to see it) and must reproduce the recorded constants; the hand-written routed
gradients equal torch autograd on per-sample tables; and the geometry the case table names (JP, jchunk, empty parts, channel blocks,
slab sets) is what ``plan_model`` -- b16_shape written out once more -- computes.

What the library itself confirms without a device: fgnn_mpconv_forward_lds_bytes answers for the generic kernel's layout whatever
family takes the call, so it cannot pin JP; fgnn_mpconv_forward_stats_partials runs the real dispatch table and returns the grid
256 * min(4, 160 KiB / LDS bytes) of the family that takes a statistics call, which pins the model's LDS bytes to a bracket for the
shapes that have a statistics epilogue (JP = 1 all of them), and shows the M k net = 1536 staging limit from both sides."""
import ctypes

import pytest
import torch

import mpconv_b16_cases as C
import mpconv_sg_cases as S

NAMES = [c[0] for c in C.FORWARD]


def runs_of(name):
    """(agg, tied) of a case's forward runs."""
    return [(agg, agg == 'max' and name in C.TIED) for agg in C.AGGS]


@pytest.mark.parametrize('name', NAMES)
def test_rounding_model_stays_within_the_derived_bound(name):
    for agg, tied in runs_of(name):
        q = C.problem(name, tied=tied)
        ref, model = C.forward_reference(q, agg), C.forward_reference(q, agg, rounded=True)
        ratio = C.bound_ratio(model['z'], ref)
        share = float((ref['bound'] / ref['z'].abs().max()).max())
        line = '%-4s %-7s model / bound %.3f, largest bound %.2e of the output range' % (name, agg, ratio, share)
        assert ratio <= 1.0, line
        assert share <= C.TOL, line                                             # the derived bound is the tighter of the two
        if agg == 'max':
            gap, named = C.argmax_gap_ratio(model['sel'], ref)
            line += ', argmax gap / (b_j + b_j*) %.3f (/ 2 b_j of the named one alone %.3f)' % (gap, named)
            assert gap <= 1.0, line
            if tied:
                assert int((model['sel'] == q['shape'][5] - 1).sum()) == 0      # first occurrence: never the copy in the last slot
        print(line)


@pytest.mark.parametrize('name', C.AFFINE)
def test_rounding_model_with_the_affine_epilogue(name):
    q = C.problem(name)
    aff = C.affine_of(q)
    assert float(aff[0].min()) < 0 < float(aff[0].max())
    for agg in C.AGGS:
        ref, model = C.forward_reference(q, agg, aff, True), C.forward_reference(q, agg, aff, True, rounded=True)
        assert 0.2 < float((ref['z'] == 0).double().mean()) < 0.8               # the ReLU cuts a real share
        assert C.bound_ratio(model['z'], ref) <= 1.0


@pytest.mark.parametrize('name', C.LARGE_BATCH)
def test_rounding_model_at_the_large_batch(name):
    q = C.problem(name, C.B_LARGE, tied=name in C.TIED)
    ref, model = C.forward_reference(q, 'max'), C.forward_reference(q, 'max', rounded=True)
    gap, named = C.argmax_gap_ratio(model['sel'], ref)
    print('%s B=%d model / bound %.3f, argmax gap / (b_j + b_j*) %.3f (/ 2 b_j of the named one alone %.3f)' % (
        name, C.B_LARGE, C.bound_ratio(model['z'], ref), gap, named))
    assert C.bound_ratio(model['z'], ref) <= 1.0 and gap <= 1.0


def test_reference_is_the_oracle():
    """The f64 expression is the oracle's mp_conv, per-sample tables and all three aggregators."""
    import fgnn_oracle as O
    for name in ('F2', 'F10', 'F9'):
        q = C.problem(name)
        nin, nou, net, N, M, k = q['shape']
        for agg in C.AGGS:
            ref = C.forward_reference(q, agg)['z']
            o = O.mp_conv({'filters': q['W'].double(), 'bias': q['bias'].double()}, '', q['x'].double().permute(0, 2, 1)[..., None],
                          q['idx'], q['et'].double().permute(0, 3, 1, 2), nou=nou, net=net, extension=0, aggregator=agg, relu=False)
            assert S.rel_err(ref, o[:, :, :, 0].permute(0, 2, 1)) <= 1e-12


def rounding_model_error(name):
    """(d_node, d_edge) of one backward case, as tests/test_mpconv_sg_cases.py measures them; also: the hand-written gradients,
    unrounded, are the autograd ones on per-sample tables."""
    q = C.problem(name)
    nin, nou, net, N, M, k = q['shape']
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
    assert int((gx[C.empty_nodes(idx, q['B'], N)] != 0).sum()) == 0
    return node, edge


@pytest.mark.parametrize('name', [n for n, _ in C.BACKWARD])
def test_rounding_model_error(name):
    d_node, d_edge = rounding_model_error(name)
    print('%-4s d_node %.4e  d_edge %.4e  (recorded: %.4e, %.4e)' % (name, d_node, d_edge, *C.D[name]))
    # the recorded yardstick is this measurement rounded up: the measurement is never above it and at most 2 % below
    assert 0.98 * C.D[name][0] <= d_node <= C.D[name][0] and 0.98 * C.D[name][1] <= d_edge <= C.D[name][1]


def test_the_table_names_what_the_plan_computes():
    pm = {n: C.plan_model(C.SHAPE[n]) for n in NAMES}
    for name, shape, jp, _ in C.FORWARD:
        assert (pm[name] is None) == (jp is None), name
        if jp is not None:
            assert pm[name]['JP'] == jp, (name, pm[name])
            assert C.forward_kernel(shape, 'max').startswith('mpconv_fwd_b16_kernel<%d, 0, ' % shape[2])
    g = lambda n, *f: tuple(pm[n][x] for x in f)
    assert g('F1', 'jchunk', 'empty_parts') == (3, 1) and g('F2', 'jchunk', 'empty_parts') == (3, 2) and 17 - 5 * 3 == 2
    assert g('F3', 'jchunk', 'units') == (48, 3) and 48 > 32                     # two blocks of 32 ids per part at net = 4
    assert g('F4', 'NPASS', 'JP', 'otc') == (2, 2, 64)
    assert g('F5', 'nch', 'KSB', 'JP') == (2, 4, 4) and g('F6', 'jchunk', 'JP') == (25, 8)
    assert g('F7', 'nch', 'SWP', 'JP') == (4, 2, 2)
    assert g('F8', 'ncols', 'SWP', 'otc') == (192, 2, 48) and (21 * 5) % 2 == 1
    assert g('F9', 'ncols', 'SWP', 'otc') == (80, 1, 20) and g('F10', 'nch', 'otc') == (2, 112)
    assert g('F11a', 'JP', 'units') == (2, 3) and g('F11b', 'JP', 'units') == (1, 5)
    assert g('F12', 'KSB', 'SWP') == (4, 2)
    assert 4 * 96 * 4 == 1536 and g('F13', 'JP', 'units') == (1, 7) and 8 * 64 == 512 and pm['F14']['JP'] == 1
    # the staging limits from the other side: one more neighbour and the kernel refuses
    assert C.plan_model((64, 64, 4, 96, 4, 97)) is None and C.plan_model((64, 64, 1, 64, 8, 65)) is None
    # a second sample per workgroup at B_LARGE: the grid is capped below it
    for n in C.LARGE_BATCH:
        assert pm[n]['grid_cap'] == 1024 < C.B_LARGE
    # every case differs from the shapes the suite already ran: nou in {64, 128} with k <= 12
    assert all(s[1] not in (64, 128) or s[5] > 12 or n in ('F12',) for n, s, _, _ in C.FORWARD)


def test_backward_families_follow_the_plan_rules():
    for name, kern in C.BACKWARD:
        assert ('mpconv_bwd_b16' in kern) == (C.backward_family(C.SHAPE[name]) == 'mpconv_bwd_b16'), name
    assert C.backward_family(C.SHAPE['E1']) != C.backward_family(C.SHAPE['E2'])         # N = 9 | 8: rule 7's lower limit
    assert C.SHAPE['E3'][5] == 255 and C.SHAPE['E3'][4] * 255 <= 512


def test_statistics_grid_brackets_the_planned_lds_bytes():
    """The real dispatch table, without a device: mpconv_fwd_b16 is the only family with a statistics epilogue for a per-sample
    table, so the row count is its grid."""
    from fgnn_amd import _hip
    L = _hip.lib()
    B = 4096

    def rows(shape):
        nin, nou, net, N, M, k = shape
        x = torch.zeros(B, N, nin, dtype=torch.bfloat16).permute(0, 2, 1).unsqueeze(-1)
        idx = torch.zeros(B, M, k, dtype=torch.int64)
        et = torch.zeros(B, M, k, net, dtype=torch.bfloat16).permute(0, 3, 1, 2)
        y = torch.zeros(B, M, nou, dtype=torch.bfloat16).permute(0, 2, 1).unsqueeze(-1)
        d = _hip.make_desc(x, idx, et, nou, net, 0, _hip.AGG_MAX, False, y)
        return L.fgnn_mpconv_forward_stats_partials(ctypes.byref(d))

    for name in ('F8', 'F9', 'F12', 'F14') + C.STATISTICS:
        pm = C.plan_model(C.SHAPE[name], stats=True)
        assert pm is not None and pm['JP'] == 1 and rows(C.SHAPE[name]) == pm['grid_cap'], (name, pm)
    assert rows((64, 64, 4, 96, 48, 7)) == 512 == C.plan_model((64, 64, 4, 96, 48, 7), True)['grid_cap']      # a 2-per-CU bracket too
    assert rows(C.SHAPE['F15']) == 0 and C.plan_model(C.SHAPE['F15']) is None       # M k net = 1600: no b16 plan
    assert rows((64, 64, 4, 30, 8, 48)) == 1024                                     # M k net = 1536: planned
    assert rows(C.SHAPE['F13']) == 0 and C.plan_model(C.SHAPE['F13'], True) is None  # (M = 4: too few destinations for the epilogue)
