"""CPU: the contract of tests/mpconv_sg_cases.py, which tests/test_mpconv_sg_irregular_gpu.py relies on.  The table generator gives
the in-degree profile it promises for every case (bound DEG, empty nodes, a node at DEG, a spread of degrees) and ``with_tied_rows``
keeps it; the share of outputs the oracle comparison leaves in stays above 0.9; the routed reference, given the oracle's own argmax,
IS the oracle's autograd (f64, 1e-10); and the per-node / per-edge yardstick D_NODE / D_EDGE is measured here (run with -s to see it)."""
import pytest
import torch

import mpconv_sg_cases as C

ALL = C.CASES + C.SWITCH_CASES
IDS = [C.case_id(c) for c in C.CASES] + ['switch-' + C.case_id(c) for c in C.SWITCH_CASES]


def has_room_for_three_degrees(N, M, k, empty):
    """Three distinct in-degrees fit: with an empty node (degree 0) and a node at DEG, one unit of slack puts a node in between;
    without one, three units make two different degrees below DEG."""
    slack = (N - empty) * C.DEG[k] - M * k
    return slack >= 1 if empty else slack >= 3


@pytest.mark.parametrize('case', ALL, ids=IDS)
@pytest.mark.parametrize('B', C.BATCHES)
def test_generator_contract(case, B):
    nin, nou, N, M, k = case[2]
    cap = C.DEG[k]
    q = C.problem(case[2], B)
    idx, deg = q['idx'], q['deg']
    assert idx.shape == (1, M, k) and idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < N
    assert torch.equal(C.in_degree(idx, N), deg)
    assert int(deg.max()) == cap                                              # within the bound, and a node exactly at it
    assert int((deg == 0).sum()) >= q['empty']
    if has_room_for_three_degrees(N, M, k, q['empty']):
        assert len(torch.unique(deg)) >= 3, deg.tolist()
    t = C.problem(case[2], B, tied=True)
    assert torch.equal(C.in_degree(t['idx'], N), deg)                         # the swaps keep the profile
    for r in t['tied']:
        assert int(t['idx'][0, r, 0]) == int(t['idx'][0, r, k - 1]) and torch.equal(t['et'][:, r, 0], t['et'][:, r, k - 1])
    assert set(t['tied']) <= set(range(0, M, C.TIE_EVERY))
    if M >= C.TIE_EVERY:                                                      # (a first node of in-degree 1 cannot be tied)
        assert len(t['tied']) >= 1, t['tied']


def test_the_case_list_covers_the_profiles_the_kernels_pad_for():
    """Over the list: tables with empty nodes for both degrees, with partly filled slot rows next to full ones, ragged N and M."""
    for k in (3, 6):
        qs = [C.problem(c[2], 37) for c in C.CASES if c[2][4] == k]
        assert sum(int((q['deg'] == 0).sum()) > 0 for q in qs) >= 3
        assert sum(len(torch.unique(q['deg'])) >= 3 for q in qs) >= 3
        assert any(c[2][2] % 16 and c[2][3] % 16 for c in C.CASES if c[2][4] == k)
    assert all((c[2][3] * c[2][4]) % 2 == 1 for c in C.CASES if c[0] == 'mpconv_bwd_b16')     # what keeps the table-driven family away


@pytest.mark.parametrize('case', ALL, ids=IDS)
@pytest.mark.parametrize('B', C.BATCHES)
def test_firm_share(case, B):
    """The oracle comparison zeroes gz where the best two messages are closer than bf16 can resolve: it must still see > 0.9 of them."""
    nin, nou, N, M, k = case[2]
    q = C.problem(case[2], B)
    share = float(C.firm_outputs(q['x'], q['idx'], q['et'], q['W'], nou).float().mean())
    print('%s B=%d firm share %.4f' % (C.case_id(case), B, share))
    assert share > 0.9, share


@pytest.mark.parametrize('case', C.CASES, ids=IDS[:len(C.CASES)])
def test_routed_reference_is_the_oracles_autograd_in_f64(case):
    """The reference checks itself: routed by the ORACLE's own argmax it reproduces the oracle's autograd."""
    nin, nou, N, M, k = case[2]
    q = C.problem(case[2], 5)
    x, et, W, bias, gz = (q[n].double() for n in ('x', 'et', 'W', 'bias', 'gz'))
    _, E = C.messages(x, q['idx'], et, W, nou)
    sel = C.first_argmax(E)
    a = C.routed_reference(x, q['idx'], et, W, bias, gz, sel, dtype=torch.float64)
    b = C.oracle_reference(x, q['idx'], et, W, bias, gz, dtype=torch.float64)
    for name, u, v in zip(('z', 'gx', 'getype', 'gW', 'gbias'), a, b):
        assert u.shape == v.shape and u.dtype == torch.float64, name
        assert C.rel_err(u, v) <= 1e-10, (name, C.rel_err(u, v))


def rounding_model_error(case, B=37):
    """(d_node, d_edge) of one case: the routed reference with the kernels' rounding points against the unrounded one (routing: the
    first largest f32 message, tied rows in).  Also: the hand-written gradients, unrounded, are the autograd ones."""
    nin, nou, N, M, k = case[2]
    q = C.problem(case[2], B, tied=True)
    x, idx, et, W, bias, gz = q['x'], q['idx'], q['et'], q['W'], q['bias'], q['gz']
    _, E = C.messages(x.float(), idx, et.float(), W, nou)
    sel = C.first_argmax(E)
    ref = C.routed_reference(x, idx, et, W, bias, gz, sel)
    plain = C.routed_by_hand(x, idx, et, W, gz, sel, rounded=False)
    for u, v in zip(plain, ref[1:]):
        assert C.rel_err(u, v) <= 1e-5
    gx, get, _, _ = C.routed_by_hand(x, idx, et, W, gz, sel, rounded=True)
    node, stray_n = C.per_row_error(gx, ref[1], (0, 2))
    edge, stray_e = C.per_row_error(get, ref[2], (0, 3))
    assert stray_n == 0 and stray_e == 0
    return node, edge


def test_rounding_model_error():
    d = [rounding_model_error(c) for c in C.CASES]
    for c, (n, e) in zip(C.CASES, d):
        print('%-22s d_node %.4e  d_edge %.4e' % (C.case_id(c), n, e))
    d_node, d_edge = max(n for n, _ in d), max(e for _, e in d)
    print('d_node %.4e  d_edge %.4e  (recorded: %.4e, %.4e)' % (d_node, d_edge, C.D_NODE, C.D_EDGE))
    # the recorded yardstick is this measurement, rounded up to two digits: neither below it nor generously above
    assert d_node <= C.D_NODE <= 1.05 * d_node and d_edge <= C.D_EDGE <= 1.05 * d_edge
