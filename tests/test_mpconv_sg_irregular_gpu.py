"""GPU: the operator backward for a batch-shared neighbour table -- the table-driven family (csrc/mpconv_bwd_ws.hip) and, where M k is
odd or behind ``FGNN_NO_WS=1``, the first-generation one (csrc/mpconv_bwd_b16.hip) -- on the graphs tests/test_mpconv_sg_gpu.py never
gives them: irregular in-degree (nodes nobody lists, whose gx row must be written as zeros; nodes below DEG next to nodes at DEG: partly
filled slot rows and their padding entries), a node listed twice by one destination, ragged N and M (the ``n < N`` / ``m < M`` guards,
the pad rows of the LDS images), and the DEG / DEG + 1 boundary of the in-degree bound the table-driven kernel trusts.  Cases, generator
and references: tests/mpconv_sg_cases.py (its contract is tests/test_mpconv_sg_cases.py, CPU).  Every case asserts the kernel family
through ``fgnn_last_kernel``, so a dispatch change cannot quietly move it elsewhere; ``FGNN_NO_WS=1`` is read once per process:
``test_first_generation_behind_the_switch`` runs the table-driven family's shapes on the first generation in one child process.

Bounds.  z and the four gradients: 2^-6 of each tensor's range, the project's bound for these kernels (P, dP and the outputs are bf16),
against the oracle's autograd (its own routing; gz zero where the best two messages are closer than bf16 resolves, > 0.9 of the outputs
left) and against torch autograd through the kernel's own argmax (tied rows in, every gz live).  Per node of gx and per edge of getype,
each over that node's / edge's OWN reference range over the batch, so that a low-degree node cannot hide behind the global maximum:
4 d, where d is the same error of the routed reference evaluated with the kernels' rounding points (P and dP held as bf16, gx and getype
stored as bf16) against the unrounded one -- measured on the CPU by ``test_mpconv_sg_cases.test_rounding_model_error`` over every case at
B = 37: d_node 4.6421e-03 (recorded as D_NODE = 4.7e-3), d_edge 5.9725e-03 (D_EDGE = 6.0e-3).  The factor 4 is for the device's other
summation order and the second bf16 rounding of gx / getype in the two-launch forms.  The device's figures are printed beside the
bounds (-s); first measured on an MI355X: worst node 5.56e-03, worst edge 8.24e-03, z and the gradients at most 6.2e-03 of their range.

What these cases found.  The degree-3 instances of the table-driven family for more than 48 nodes (64x64x64x96x3, 64x64x50x64x3,
128x64x50x64x3) had never run: the 64-channel calls were turned down by the node limit of a second kernel generation (since deleted)
whose rules the plan then shared, and the kernel staged the edge types of the first 384 in-edge slots only (48 nodes of 8 slots), so
gx of nodes 48.. was zero (worst node 1.0) and gW was off by half its range.  Those cases are the regression test.

The moved cases on mpconv_bwd_b16 (first measured on an MI355X): the three with an odd M k and the four behind FGNN_NO_WS=1 give z and
the gradients at most 4.3e-03 of their range, worst node 4.94e-03, worst edge 5.97e-03."""
import json
import os
import subprocess
import sys

import pytest
import torch

import mpconv_sg_cases as C

pytestmark = pytest.mark.gpu

IDS = [C.case_id(c) for c in C.CASES]
NODE_BOUND, EDGE_BOUND = 4 * C.D_NODE, 4 * C.D_EDGE
FAST = ('mpconv_bwd_ws',)


def by_shape(shape):
    return next(c for c in C.CASES if c[2] == shape)


@pytest.fixture(scope='module')
def routed(dev):
    """One device run and one reference per (case, B), shared by the tests that read it."""
    made = {}

    def get(case, B):
        if (case, B) not in made:
            made[case, B] = C.run_case(case, B, dev, 'routed')
        return made[case, B]
    return get


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
@pytest.mark.parametrize('B', C.BATCHES)
def test_irregular_backward_vs_oracle_autograd(case, B, dev):
    out = C.run_case(case, B, dev, 'oracle')
    print('%s B=%d %s: firm %.4f, errors z %.2e gx %.2e getype %.2e gW %.2e gbias %.2e (bound %.2e)' % (
        out['case'], B, out['kern'], out['firm'], out['err_z'], out['err_gx'], out['err_getype'], out['err_gW'], out['err_gbias'], C.TOL))
    C.check(out)


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
@pytest.mark.parametrize('B', C.BATCHES)
def test_irregular_backward_vs_routed_reference_with_tied_rows(case, B, routed):
    """Every gz live, rows ::5 list their first node again in the last slot with the same edge types.  gx of a node nobody lists is
    zero in every bit and gx is finite everywhere; in a tied row the slot the argmax names gets the edge-type gradient, the other one
    nothing (the reference's own getype on those rows; the two slots differ wherever the reference's do)."""
    out = routed(case, B)
    print('%s B=%d %s: %d empty nodes, %d tied rows (%d entries differ), errors z %.2e gx %.2e getype %.2e gW %.2e gbias %.2e, tied %.2e '
          '(bound %.2e)' % (out['case'], B, out['kern'], out['empty_nodes'], out['tied_rows'], out.get('tied_differ', 0), out['err_z'],
                            out['err_gx'], out['err_getype'], out['err_gW'], out['err_gbias'], out.get('tied_err', 0.0), C.TOL))
    C.check(out)
    assert out['empty_nodes'] >= C.empties_for(*case[2][2:])
    if case[2][3] >= C.TIE_EVERY:
        assert out['tied_rows'] >= 1 and out['tied_differ'] > 0, out


@pytest.mark.parametrize('case', C.CASES, ids=IDS)
@pytest.mark.parametrize('B', C.BATCHES)
def test_irregular_backward_per_node_and_per_edge(case, B, routed):
    out = routed(case, B)
    print('%s B=%d %s: worst node of gx %.4e (bound %.4e = 4 x %.4e), worst edge of getype %.4e (bound %.4e = 4 x %.4e)' % (
        out['case'], B, out['kern'], out['node_err'], NODE_BOUND, C.D_NODE, out['edge_err'], EDGE_BOUND, C.D_EDGE))
    C.check(out, NODE_BOUND, EDGE_BOUND)


@pytest.mark.parametrize('shape', [(64, 64, 91, 45, 6), (64, 64, 37, 60, 3), (64, 128, 91, 40, 6)], ids=lambda s: 'x'.join(map(str, s)))
def test_irregular_backward_with_prebuilt_tables_is_bit_identical(shape, dev):
    """ops.BACKWARD_TABLES: the transposed incidence built once per graph by its own small kernel == what every workgroup builds for
    itself, padding entries and empty nodes included: all four gradients bit-identical."""
    case = by_shape(shape)
    a, b = C.run_case(case, 37, dev, 'routed', tables=True), C.run_case(case, 37, dev, 'routed', tables=False)
    assert a['built_tables'] and not b['built_tables']
    assert 'mpconv_bwd_ws' in a['kern'] and a['kern'] == b['kern']
    for u, v in zip(a['grads'], b['grads']):
        assert torch.equal(u, v)


def _bounded_below_cap(shape, seed):
    """A case's inputs with a table whose largest in-degree is DEG - 1, and its in-degrees."""
    nin, nou, N, M, k = shape
    g = torch.Generator().manual_seed(seed)
    idx, deg = C.bounded_table(N, M, k, C.DEG[k] - 1, g, 0)
    q = C.problem(shape, 37)
    q['idx'] = idx
    return q, deg


def _against_routed(q, idx, dev, idx_dev):
    x, et, W, bias, gz = q['x'], q['et'], q['W'], q['bias'], q['gz']
    z, am, gx, get, gW, gb, kern = C.device_backward(x, idx, et, W, bias, gz, dev, idx_dev=idx_dev)
    r = C.routed_reference(x, idx, et, W, bias, gz, am)
    errs = [C.rel_err(a, b) for a, b in zip((z, gx, get, gW, gb), r)]
    return kern, errs, (gx, get, gW, gb)


# M k <= N (DEG - 1): room for a table that stays below the cap
BOUNDARY_SHAPES = [(64, 64, 96, 30, 6), (64, 64, 37, 60, 3), (64, 64, 64, 96, 3), (64, 128, 91, 30, 6)]
ODD_SHAPE = (64, 64, 37, 59, 3)            # M k odd: mpconv_bwd_b16, which takes any in-degree


@pytest.mark.parametrize('shape', BOUNDARY_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_in_degree_boundary_and_remeasurement_after_an_in_place_edit(shape, dev):
    """The table-driven kernel drops an in-edge beyond DEG without a word, so the bound the caller measured (ops.max_in_degree, remembered on the
    tensor) must be right: one entry edited so that a node has exactly DEG in-edges -> still a fast family; the SAME device tensor
    edited in place to DEG + 1 -> the remembered value is measured again and the call goes to mpconv_bwd_b16.  Both within 2^-6 of
    the routed reference."""
    from fgnn_amd import ops
    nin, nou, N, M, k = shape
    cap = C.DEG[k]
    q, deg = _bounded_below_cap(shape, 11 + N + M)
    idx = q['idx'].clone()
    flat = idx[0].reshape(-1)
    a = int((deg == cap - 1).nonzero()[0])
    donors = [p for p in range(M * k) if int(flat[p]) != a and int(deg[flat[p]]) >= 2][:2]       # (their nodes stay listed)
    assert int(deg.max()) == cap - 1 and len(donors) == 2
    idx_dev = idx.to(dev)
    assert ops.max_in_degree(idx_dev.expand(37, -1, -1), N) == cap - 1
    names = []
    for step, want in ((0, cap), (1, cap + 1)):
        flat[donors[step]] = a
        idx_dev[0].view(-1)[donors[step]] = a                                                  # in place: the version changes
        assert int(C.in_degree(idx, N).max()) == want
        kern, errs, _ = _against_routed(q, idx, dev, idx_dev)
        print('%s in-degree %d: %s, errors z %.2e gx %.2e getype %.2e gW %.2e gbias %.2e' % ('x'.join(map(str, shape)), want, kern, *errs))
        names.append(kern)
        assert ops.max_in_degree(idx_dev.expand(37, -1, -1), N) == want
        assert max(errs) <= C.TOL, (kern, errs)
    assert any(f in names[0] for f in FAST), names
    assert 'mpconv_bwd_b16' in names[1], names


@pytest.mark.parametrize('shape', BOUNDARY_SHAPES[:3] + [ODD_SHAPE], ids=lambda s: 'x'.join(map(str, s)))
def test_out_of_range_ids_are_clamped(shape, dev):
    """The kernels clamp neighbour ids into [0, N): a table holding -1 and N in a few slots gives the gradients of the same table with
    0 and N - 1 written there, bit for bit -- including when the clamp is what brings node 0 to exactly DEG in-edges.  The shape with
    an odd M k runs mpconv_bwd_b16 (and mpconv_fwd_b16), which clamp when they stage the table."""
    from fgnn_amd import ops
    nin, nou, N, M, k = shape
    cap = C.DEG[k]
    q, deg = _bounded_below_cap(shape, 23 + N + M)
    idx = q['idx'].clone()
    flat = idx[0].reshape(-1)
    a = int((deg == cap - 1).nonzero()[0])                                     # relabel: node 0 is one of those at DEG - 1
    was0, wasa = flat == 0, flat == a
    flat[was0], flat[wasa] = a, 0
    deg = C.in_degree(idx, N)
    assert int(deg[0]) == cap - 1 and int(deg.max()) == cap - 1
    donors = [p for p in range(M * k) if int(flat[p]) not in (0, N - 1) and int(deg[flat[p]]) >= 2]
    low, high = donors[0], donors[-1]                                          # one slot to -1 (node 0 lands exactly on DEG), one to N
    clean, raw = idx.clone(), idx.clone()
    clean[0].view(-1)[low], raw[0].view(-1)[low] = 0, -1
    clean[0].view(-1)[high], raw[0].view(-1)[high] = N - 1, N
    assert int(C.in_degree(clean, N)[0]) == cap and int(C.in_degree(clean, N).max()) == cap
    assert int(raw.min()) == -1 and int(raw.max()) == N
    raw_dev = raw.to(dev)
    assert ops.max_in_degree(raw_dev.expand(37, -1, -1), N) == cap
    k1, e1, g1 = _against_routed(q, clean, dev, clean.to(dev))
    x, et, W, bias, gz = q['x'], q['et'], q['W'], q['bias'], q['gz']
    out = C.device_backward(x, clean, et, W, bias, gz, dev, idx_dev=raw_dev)
    assert ('mpconv_bwd_b16' if shape == ODD_SHAPE else 'mpconv_bwd_ws') in k1 and out[6] == k1, (k1, out[6])
    assert max(e1) <= C.TOL, e1
    for u, v in zip(g1, out[2:6]):
        assert torch.equal(u, v)


def test_first_generation_behind_the_switch(dev):
    """FGNN_NO_WS=1 is read once per process: ONE child process (started fresh, nothing else on the device beside it) runs cases the
    table-driven family takes in this process against both references; every one must go to mpconv_bwd_b16."""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mpconv_sg_cases.py')
    env = dict(os.environ, FGNN_NO_WS='1')
    r = subprocess.run([sys.executable, helper, '--set', 'switch', '--B', '37', '--refs', 'oracle,routed'], env=env, timeout=300,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    outs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith('{')]
    assert [(o['case'], o['ref']) for o in outs] == [(C.case_id(c), ref) for c in C.SWITCH_CASES for ref in ('oracle', 'routed')]
    for o in outs:
        print('%s %s %s: errors z %.2e gx %.2e getype %.2e gW %.2e gbias %.2e (bound %.2e)' % (
            o['case'], o['ref'], o['kern'], o['err_z'], o['err_gx'], o['err_getype'], o['err_gW'], o['err_gbias'], C.TOL)
            + ('' if o['ref'] == 'oracle' else ', worst node %.4e (bound %.4e), worst edge %.4e (bound %.4e)' % (
                o['node_err'], NODE_BOUND, o['edge_err'], EDGE_BOUND)))
        C.check(o, NODE_BOUND, EDGE_BOUND)
    assert all('mpconv_bwd_b16' in o['kern'] for o in outs), [o['kern'] for o in outs]
