"""GPU: every weight-gradient kernel of the node-wise maps through fgnn_linear_wgrad, at the cases of tests/wgrad_cases.py (whose
contract tests/test_wgrad_cases.py checks on the CPU).  Per case and data set: the kernel the library names for the real pointers is
the one the case is meant to reach; the exact sets come back EQUAL to the float64 reference (torch.equal, no tolerance); ``rand``
stays within the project's bound; a second run is bit-identical; and nothing outside gW / gb is written -- 4 KB guards either side of
every buffer, NaN around the operands, a NaN bit pattern around the outputs and all through the workspace.

Run with -s for the measured ``rand`` errors (DESIGN §7.1 records the worst per family)."""
import pytest
import torch

import wgrad_cases as C

pytestmark = pytest.mark.gpu

GUARD = 4096                            # bytes either side of every buffer
PATTERN = 0x7FC5A5A5                    # a quiet NaN as f32: a slab element read before it was written poisons the result


def _operand(t, off, dev):
    """``t`` [R, C] as a slice of a NaN-filled buffer: 4 KB, ``off`` elements, the payload, 4 KB."""
    g = GUARD // t.element_size()
    buf = torch.full((g + off + t.numel() + g,), float('nan'), dtype=t.dtype, device=dev)
    view = buf[g + off:g + off + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _output(n, value, dev):
    """n f32 holding ``value`` inside an int32 buffer of PATTERN (value None: the payload keeps the pattern too)."""
    g = GUARD // 4
    buf = torch.full((g + n + g,), PATTERN, dtype=torch.int32, device=dev)
    view = buf[g:g + n].view(torch.float32)
    if value is not None:
        view.fill_(value)
    return buf, view


def _guards_intact(buf, n):
    g = GUARD // 4
    return bool((buf[:g] == PATTERN).all()) and bool((buf[g + n:] == PATTERN).all())


def _run(L, _hip, c, xv, gyv, dev):
    R, cin, cout = c['shape']
    nws = int(L.fgnn_linear_wgrad_workspace_bytes(R, cin, cout))
    assert nws > 0 and nws % 4 == 0
    wbuf, gw = _output(cout * cin, C.GW0, dev)
    bbuf, gb = _output(cout, C.GB0, dev)
    sbuf, ws = _output(nws // 4, None, dev)
    P = _hip._ptr
    _hip.check(L.fgnn_linear_wgrad(P(xv), P(gyv), R, cin, cout, _hip.dtype_code(xv), P(gw), None if c['gb_null'] else P(gb),
                                   P(ws), nws, _hip.stream_ptr()))
    torch.cuda.synchronize()
    assert _guards_intact(wbuf, cout * cin) and _guards_intact(bbuf, cout) and _guards_intact(sbuf, nws // 4), 'a write outside a buffer'
    return gw.view(cout, cin).clone(), gb.clone()


@pytest.mark.parametrize('cid', [c['id'] for c in C.CASES])
def test_weight_gradient_kernel_vs_float64(cid, dev):
    from fgnn_amd import _hip
    L = _hip.lib()
    c = C.BY_ID[cid]
    R, cin, cout = c['shape']
    for name in C.data_sets(c):
        x, gy = C.make(c, name)
        xbuf, xv = _operand(x, c['xoff'], dev)
        gbuf, gyv = _operand(gy, c['gyoff'], dev)
        kernel = _hip.invoke('fgnn_linear_wgrad_kernel', R, cin, cout, _hip.dtype_code(xv), xv.data_ptr() & 15, gyv.data_ptr() & 15)
        assert kernel.decode() == c['kernel'], (name, c['reaches'])
        ref_w, ref_b = C.reference(xv, gyv)
        gw, gb = _run(L, _hip, c, xv, gyv, dev)
        dw, db = gw.double() - C.GW0 - ref_w, gb.double() - C.GB0 - (0 if c['gb_null'] else ref_b)
        if c['gb_null']:
            assert torch.equal(db, torch.zeros_like(db)), (name, 'gb is NULL: nothing may be added anywhere')
        if name == 'rand':
            ew, bw = float(dw.abs().max()), C.rand_bound(c, ref_w)
            eb, bb = float(db.abs().max()), C.rand_bound(c, ref_b)
            print('\n%-5s %-7s %-40s gW %.3e / %.3e  gb %.3e / %.3e' % (cid, c['family'], c['kernel'], ew, bw, eb, bb))
            assert ew <= bw and eb <= bb, (name, ew, bw, eb, bb)
        else:
            bad = dw != 0
            assert not bool(bad.any()), '%s: %d of %d gW elements differ from the exact result, the first at %s by %s' % (
                name, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(dw[bad][0]))
            assert not bool((db != 0).any()), '%s: gb differs from the exact result by up to %s' % (name, float(db.abs().max()))
        gw2, gb2 = _run(L, _hip, c, xv, gyv, dev)
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2), (name, 'a second run differs')
        assert torch.equal(xv.cpu(), x) and torch.equal(gyv.cpu(), gy), (name, 'an operand was written')
        del xbuf, gbuf


@pytest.mark.parametrize('dtype,shape', C.REFUSED, ids=['f32', 'bf16'])
def test_wider_than_the_register_tiling_is_refused_before_any_launch(dtype, shape, dev):
    from fgnn_amd import _hip
    L = _hip.lib()
    R, cin, cout = shape
    x = torch.zeros(R, cin, device=dev, dtype=C.DTYPE[dtype])
    gy = torch.zeros(R, cout, device=dev, dtype=C.DTYPE[dtype])
    wbuf, gw = _output(cout * cin, C.GW0, dev)
    sbuf, ws = _output(1 << 20, None, dev)
    P = _hip._ptr
    assert _hip.invoke('fgnn_linear_wgrad_kernel', R, cin, cout, _hip.dtype_code(x), 0, 0) == b''
    rc = L.fgnn_linear_wgrad(P(x), P(gy), R, cin, cout, _hip.dtype_code(x), P(gw), None, P(ws), 4 << 20, _hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _hip.EUNSUPPORTED
    assert bool((gw == C.GW0).all()) and bool((sbuf == PATTERN).all()) and _guards_intact(wbuf, cout * cin)
