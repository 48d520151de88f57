"""The catch-all bf16 operator kernels (csrc/mpconv_fwd_b16.hip, csrc/mpconv_bwd_b16.hip) away from the LDPC shapes: the case list, the
input generator, the references and the bounds that tests/test_mpconv_b16_cases.py (CPU) and tests/test_mpconv_b16_gpu.py (GPU) share.
A helper module like tests/mpconv_sg_cases.py, whose references it reuses (``messages``, ``routed_reference``, ``routed_by_hand``,
``per_row_error``, ``rel_err``); not a test module.

Layouts (the natural ones, channel / edge type last): x [B, N, nin], et [B, M, k, net], gz / z [B, M, nou], W [nin, nou * net] (column
o * net + e), idx [B, M, k] (per-sample tables, which keep the table-driven family away) or [1, M, k] (``shared``).

The forward bound is derived per element, not a share of the tensor's range.  With u = 2^-8 and, for an edge j of an output element,

    b_j = u sum_e |et_e| |P_e|  +  nin 2^-24 sum_e |et_e| (|x| . |W|)_e

(the bf16 rounding of P; the f32 accumulation order of the projection), the element's bound is (1 + u) agg_b + u |z_ref| with
agg_b = max_j b_j for max and softmax (the weights of a log-sum-exp's derivative sum to 1) and mean_j b_j for mean.  A post-scale
multiplies the first term by |post_scale|; z_ref is the final value.  ``rounding_model`` (P and the output rounded to bf16, everything
else f64) must stay within it on the CPU for every case: a case whose model exceeds 1.0 means a wrong bound."""
import torch

import mpconv_sg_cases as S

U = 2.0 ** -8                           # the unit the bound is written in
TOL = S.TOL                             # the project's 2^-6 of range: the ceiling over the derived bound, and the gradients' bound
AGGS = ('max', 'softmax', 'mean')
B_SMALL, B_LARGE = 6, 1029              # 1029: the grid cap of 1024 (small-LDS shapes) makes five workgroups take a second sample

# (id, (nin, nou, net, N, M, k), JP as b16_shape computes it today (None: not planned by mpconv_fwd_b16), what the case reaches)
FORWARD = [
    ('F1', (64, 64, 4, 40, 1, 20), 8, 'jchunk 3, the last part empty'),
    ('F2', (64, 64, 4, 40, 1, 17), 8, 'jchunk 3, parts 6 and 7 empty, part 5 short'),
    ('F3', (64, 64, 4, 96, 2, 96), 2, 'jchunk 48: two JB blocks of ids and weights per part'),
    ('F4', (64, 128, 4, 50, 2, 33), 2, 'NPASS 2: the red region reused per column pass'),
    ('F5', (128, 128, 1, 40, 1, 130), 4, 'hyper rule 2 -> b16, nch 2'),
    ('F6', (64, 64, 1, 130, 1, 200), 8, 'N > 128: hyper rule 3 -> b16, jchunk 25'),
    ('F7', (64, 256, 1, 33, 1, 40), 2, 'nch 4, SWP 2'),
    ('F8', (64, 48, 4, 37, 21, 5), 1, 'ncols 192 (partial second slab set), otc 48, odd M k, runtime k'),
    ('F9', (64, 20, 4, 23, 9, 4), 1, 'ncols 80 (waves 5-7 without projection work), otc 20'),
    ('F10', (64, 112, 1, 50, 7, 9), 1, 'net 1 with M > 1, nch 2 with 48 live lanes'),
    ('F11a', (64, 64, 1, 60, 2, 40), 2, 'net 1, split in two'),
    ('F11b', (64, 64, 1, 60, 3, 40), 1, 'net 1, one wave walks 40 neighbours'),
    ('F12', (128, 64, 4, 91, 47, 4), 1, 'KSB 4, runtime k, ragged N and M'),
    ('F13', (64, 64, 4, 96, 4, 96), 1, 'M k net = 1536 exactly, k = 96 unsplit'),
    ('F14', (64, 64, 1, 64, 8, 64), 1, 'M k = 512 exactly'),
    ('F15', (64, 64, 4, 30, 8, 50), None, 'M k net = 1600: mpconv_fwd_b16 refuses; another forward writes the argmax mpconv_bwd_b16 routes by'),
]
SHAPE = {c[0]: c[1] for c in FORWARD}
TIED = ('F1', 'F3', 'F4', 'F5', 'F6')   # max runs: every destination lists its slot-0 node again in slot k - 1 (different parts of the split)
LARGE_BATCH = ('F1', 'F8')
SHARED_TABLE = ('F3', 'F7')             # batch-shared table (expand): k not in {3, 6} still lands on mpconv_fwd_b16
AFFINE = ('F4', 'F7')                   # once more with bias, post_scale, post_shift and ReLU
STATISTICS = ('F8', 'F9')               # training-mode mp_conv_v2: the statistics epilogue at nou < 64

# Backward.  fgnn_bwd_b16_plan's rules 2 and 7 name the family (``backward_family``); the calls it turns down go on down the dispatch
# table: the resident family (mpconv_bwd_res.hip) takes max calls with nou a multiple of 32 channels per pass or one pass of <= 32
# (F9, the N = 8 case and the plain-layout runs), the generic kernel the rest (F8: 48 channels in two passes; softmax and mean).
BWD_EDGES = {'E1': (64, 64, 4, 9, 5, 16), 'E2': (64, 64, 4, 8, 5, 16), 'E3': (64, 64, 4, 40, 2, 255)}
SHAPE.update(BWD_EDGES)
BACKWARD = [
    ('F1', 'mpconv_bwd_b16_kernel<2, 2>'), ('F2', 'mpconv_bwd_b16_kernel<2, 2>'), ('F3', 'mpconv_bwd_b16_kernel<2, 2>'),
    ('F4', 'mpconv_bwd_b16_kernel<2, 4>'), ('F8', 'mpconv_bwd_kernel<bf16_t, 4, 0>'), ('F9', 'mpconv_bwd_res_kernel<bf16_t, 4, '),
    ('F12', 'mpconv_bwd_b16_kernel<4, 2>'), ('F13', 'mpconv_bwd_b16_kernel<2, 2>'), ('F15', 'mpconv_bwd_b16_kernel<2, 2>'),
    ('E1', 'mpconv_bwd_b16_kernel<2, 2>'), ('E2', 'mpconv_bwd_res_kernel<bf16_t, 4, '), ('E3', 'mpconv_bwd_b16_kernel<2, 2>'),
]
BACKWARD_PLAIN = [('F1', 'mpconv_bwd_res_kernel<bf16_t, 4, '), ('F12', 'mpconv_bwd_res_kernel<bf16_t, 4, ')]   # rule 6 turns them down
BACKWARD_ORACLE = ('F8', 'F10', 'F11a', 'F11b')        # softmax and mean: the generic backward, against the oracle's own autograd

# Per-node / per-edge yardstick of the backward cases, as tests/mpconv_sg_cases.py defines D_NODE / D_EDGE: the routed reference with
# the kernels' rounding points (P and dP held as bf16, gx and getype stored as bf16) against the unrounded one, each node's / edge's
# error over its OWN reference range over the batch, at B = 6 -- measured on the CPU by
# tests/test_mpconv_b16_cases.py::test_rounding_model_error, which asserts these values hold.  Per case: an edge of F13 (k = 96, four
# destinations) is routed by one or two channels of the batch, so its range is small and its d four times that of the others; one
# constant for the list would leave the other cases a bound that wide.  (d_node, d_edge), the measurement rounded up by about 1 %:
D = {
    'F1':  (4.73e-03, 4.58e-03),        # measured 4.6892e-03, 4.5399e-03
    'F2':  (5.90e-03, 5.24e-03),        # measured 5.8512e-03, 5.1943e-03
    'F3':  (5.29e-03, 8.28e-03),        # measured 5.2416e-03, 8.2126e-03
    'F4':  (4.53e-03, 6.54e-03),        # measured 4.4897e-03, 6.4797e-03
    'F8':  (4.54e-03, 5.89e-03),        # measured 4.5037e-03, 5.8337e-03
    'F9':  (3.99e-03, 4.55e-03),        # measured 3.9487e-03, 4.5103e-03
    'F12': (4.28e-03, 6.80e-03),        # measured 4.2408e-03, 6.7364e-03
    'F13': (4.96e-03, 1.89e-02),        # measured 4.9158e-03, 1.8706e-02
    'F15': (4.46e-03, 9.06e-03),        # measured 4.4208e-03, 8.9804e-03
    'E1':  (3.70e-03, 6.45e-03),        # measured 3.6675e-03, 6.3945e-03
    'E2':  (3.76e-03, 7.57e-03),        # measured 3.7301e-03, 7.5098e-03
    'E3':  (4.49e-03, 6.12e-03),        # measured 4.4519e-03, 6.0673e-03
}


def plan_model(shape, stats=False):
    """b16_shape / b16_widths of csrc/mpconv_fwd_b16.hip written out once more, AS CODED TODAY (``units`` multiplies before it
    divides): a dict with the geometry the table above names, or None where the kernel refuses the shape.  No entry point reports
    JP or this kernel's LDS bytes without a device (fgnn_mpconv_forward_lds_bytes answers for the generic kernel's layout whatever
    family takes the call), so this is the table's arithmetic, checked against the library only through the statistics grid."""
    nin, nou, net, N, M, k = shape
    ncols, mk = nou * net, M * k
    if net not in (1, 4) or ncols % 16 or ncols > 512 or nin not in (64, 128):
        return None
    if nin * N // 8 > 512 * 3 or mk * net > 512 * 3 or mk > 512:
        return None
    if stats and net == 1 and (M == 1 or (N == 1 and k == 1)):
        return None
    npass = (ncols + 255) // 256
    if npass > 1 and ncols % 256:
        return None
    if stats and (npass != 1 or nou > 64 or M * ((nou + 63) // 64) * 2 <= 8):
        return None
    pass_cols = ncols if npass == 1 else 256
    ksb, swp = nin // 32, (pass_cols // 16 + 7) // 8
    if (ksb, swp, npass) not in ((2, 1, 1), (2, 2, 1), (2, 2, 2), (4, 1, 1), (4, 2, 1)):
        return None
    up = lambda v, m: (v + m - 1) // m * m
    Npad = up(N, 16)
    lds = up(Npad * (nin * 2 + 16), 16)
    lds = up(lds + Npad * (pass_cols * 2 + 16), 16)
    lds += up(mk, 4) * 4 + up(mk * net * 2, 16)
    otp = pass_cols // net
    units = M * (min(otp, nou) + 63) // 64
    jp = 8 // units if k >= 16 and units * 2 <= 8 else 1
    if jp > 1:
        lds += units * jp * 768
    if lds > 160 * 1024:
        return None
    jchunk = (k + jp - 1) // jp
    otc = min(otp, nou)
    return dict(JP=jp, jchunk=jchunk, empty_parts=sum(1 for q in range(jp) if q * jchunk >= k), units=units, ncols=ncols, NPASS=npass,
                KSB=ksb, SWP=swp, otc=otc, nch=(otc + 63) // 64, lds=lds, grid_cap=256 * max(1, min(4, 160 * 1024 // lds)))


def forward_kernel(shape, agg):
    """The name fgnn_last_kernel must report for a forward case: mpconv_fwd_b16 with the template arguments of the plan, or (F15 and
    E3, whose M k net is beyond its staging registers) the resident kernel's prefix."""
    pm = plan_model(shape)
    if pm is None:
        return 'mpconv_fwd_res_kernel<bf16_t, %d, %d, ' % (shape[2], AGGS.index(agg))
    kc = shape[5] if (agg == 'max' and shape[2] == 4 and shape[5] in (3, 6)) else 0
    return 'mpconv_fwd_b16_kernel<%d, %d, %d, %d, %d, %d>' % (shape[2], AGGS.index(agg), pm['KSB'], pm['SWP'], pm['NPASS'], kc)


def backward_family(shape):
    """fgnn_bwd_b16_plan's rules 2, 3, 7 and 10 for a bf16, channel-fastest, edge-type-fastest, max, 4-edge-type call."""
    nin, nou, net, N, M, k = shape
    ok = (net == 4 and nin in (64, 128) and nou in (64, 128) and (nin, nou) != (128, 128) and 9 <= N <= 96 and M * k <= 512
          and 2 <= k <= 255 and M <= 128)
    return 'mpconv_bwd_b16' if ok else 'other'


def problem(name, B=B_SMALL, tied=False, shared=False, seed=0):
    """The inputs of one case as CPU tensors (bf16 values held as bf16; W holds bf16 values in f32): a dict.  ``tied``: every
    destination lists its slot-0 node again in slot k - 1 with the same edge types -- two messages that are bit-equal in the kernel."""
    nin, nou, net, N, M, k = SHAPE[name]
    g = torch.Generator().manual_seed(seed + 2000 + N + 7 * M + 13 * nou + 17 * k + nin + net + B)
    x = torch.randn(B, N, nin, generator=g).bfloat16()
    idx = torch.randint(0, N, (1 if shared else B, M, k), generator=g)
    et = torch.randn(B, M, k, net, generator=g).bfloat16()
    W = (torch.randn(nin, nou * net, generator=g) * 0.1).bfloat16().float()
    bias = torch.randn(nou, generator=g)
    gz = torch.randn(B, M, nou, generator=g).bfloat16()
    if tied:
        idx[:, :, k - 1] = idx[:, :, 0]
        et[:, :, k - 1, :] = et[:, :, 0, :]
    return dict(name=name, shape=SHAPE[name], B=B, x=x, idx=idx, et=et, W=W, bias=bias, gz=gz, tied=tied, shared=shared)


def affine_of(q):
    """(post_scale, post_shift) [nou] of a case's epilogue run: both signs in equal shares, so that the ReLU cuts about half."""
    g = torch.Generator().manual_seed(77 + q['shape'][1])
    return torch.randn(q['shape'][1], generator=g), torch.randn(q['shape'][1], generator=g)


def empty_nodes(idx, B, N):
    """[B, N] bool: nodes no destination of that sample lists."""
    idx = idx.expand(B, -1, -1)
    listed = torch.zeros(B, N, dtype=torch.bool)
    listed[torch.arange(B)[:, None], idx.reshape(B, -1)] = True
    return ~listed


# ----------------------------------------------------------------------------------------------------------------------------------
# the forward's reference, bound and rounding model (f64)
# ----------------------------------------------------------------------------------------------------------------------------------
def _aggregate(E, b, agg):
    if agg == 'max':
        return E.amax(2), b.amax(2)
    if agg == 'softmax':
        return torch.logsumexp(3.0 * E, 2) / 3.0, b.amax(2)         # the oracle's LSE_GAMMA = 3
    return E.mean(2), b.mean(2)


def _finish(a, q, affine, relu):
    z = a + q['bias'].double()
    scale = None
    if affine is not None:
        scale = affine[0].double()
        z = z * scale + affine[1].double()
    return (z.clamp_min(0.0) if relu else z), scale


def forward_reference(q, agg, affine=None, relu=False, rounded=False, chunk=64):
    """f64 on the case's bf16-rounded x, et and W: dict(z, bound [B, M, nou], E, b [B, M, k, nou] the per-edge messages and their
    bounds).  ``rounded``: the rounding model instead -- P and the output rounded to bf16 -- with ``sel``, its first-occurrence argmax."""
    nin, nou, net, N, M, k = q['shape']
    out = dict(z=[], bound=[], E=[], b=[], sel=[])
    W = q['W'].double()
    for lo in range(0, q['B'], chunk):
        x, et = q['x'][lo:lo + chunk].double(), q['et'][lo:lo + chunk].double()
        idx = q['idx'] if q['idx'].shape[0] == 1 else q['idx'][lo:lo + chunk]
        P = torch.einsum('bnc,cq->bnq', x, W).reshape(-1, N, nou, net)
        A = torch.einsum('bnc,cq->bnq', x.abs(), W.abs()).reshape(-1, N, nou, net)
        Pg, ea = S.rows_of(P, idx), et.abs()[:, :, :, None, :]
        b = U * (Pg.abs() * ea).sum(-1) + nin * 2.0 ** -24 * (S.rows_of(A, idx) * ea).sum(-1)
        if rounded:
            Pg = S.rows_of(P.bfloat16().double(), idx)
        E = (Pg * et[:, :, :, None, :]).sum(-1)
        a, agg_b = _aggregate(E, b, agg)
        z, scale = _finish(a, q, affine, relu)
        if rounded:
            z = z.bfloat16().double()
            out['sel'].append(S.first_argmax(E))
        out['bound'].append((1.0 + U) * agg_b * (1.0 if scale is None else scale.abs()) + U * z.abs())
        out['z'].append(z), out['E'].append(E), out['b'].append(b)
    return {n: torch.cat(v) for n, v in out.items() if v}


def bound_ratio(z, ref):
    """The worst element's error over its own derived bound."""
    return float(((z.double() - ref['z']).abs() / ref['bound']).max())


def argmax_gap_ratio(am, ref):
    """Max aggregator: how far below the true f64 maximum the named neighbour's f64 message lies, over the slack the rounding of P
    allows.  The kernel prefers j to the maximiser j* only if their rounded messages say so, and each moved by at most its own b, so
    E[j*] - E[j] <= b_j + b_j* -- "2 b_j" with the two neighbours' own bounds.  Twice the NAMED neighbour's bound alone is not a bound:
    the rounding model, a correct implementation, reaches 1.61 of it (F8 at B = 1029, where b_j* > b_j).  Returns
    (worst gap / (b_j + b_j*), worst gap / (2 b_j), the latter for the record)."""
    am = am.long()[:, :, None, :]
    E, b = ref['E'], ref['b']
    top, jstar = E.max(2, keepdim=True)
    gap = (top - E.gather(2, am))[:, :, 0, :]
    bj, bs = b.gather(2, am)[:, :, 0, :], b.gather(2, jstar)[:, :, 0, :]
    return float((gap / (bj + bs)).max()), float((gap / (2.0 * bj)).max())


# ----------------------------------------------------------------------------------------------------------------------------------
# the device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _operands(q, dev, layout):
    """x [B, nin, N, 1] channel-fastest, the table (a stride-0 view where shared), et [B, net, M, k] in one of the two layouts."""
    B = q['B']
    xd = q['x'].to(dev)[:, :, None, :].permute(0, 3, 1, 2)
    etd = q['et'].to(dev).permute(0, 3, 1, 2)                                      # edge-type fastest: stored [B, M, k, net]
    if layout == 'plain':
        etd = etd.contiguous()                                                     # stored [B, net, M, k]
    return xd, q['idx'].to(dev).expand(B, -1, -1), etd


def device_forward(q, agg, dev, layout='fastest', affine=None, relu=False, bias=True):
    """One forward launch: (z [B, M, nou] as stored (bf16 held in f32), argmax [B, M, nou] or None, kernel name), on the CPU."""
    from fgnn_amd import _hip, ops
    nin, nou, net, N, M, k = q['shape']
    xd, idxd, etd = _operands(q, dev, layout)
    kw = {} if affine is None else dict(post_scale=affine[0].to(dev), post_shift=affine[1].to(dev))
    y, am = ops.mpconv_forward_raw(xd, idxd, etd, q['W'].to(dev), q['bias'].to(dev) if bias else None, nou, net, 0, _hip.AGG_CODES[agg],
                                   relu=relu, want_argmax=True, **kw)
    kern = _hip.lib().fgnn_last_kernel().decode()
    assert y.dtype == torch.bfloat16 and y.stride(1) == 1
    nat = lambda t: t.cpu()[:, :, :, 0].permute(0, 2, 1)
    return nat(y.float()), (None if am is None else nat(am).long()), kern


def device_backward(q, agg, dev, layout='fastest'):
    """Forward and backward through ops.mpconv: (z, argmax or None, gx, getype, gW, gbias, the forward's kernel, the backward's), tensors
    on the CPU in this module's layouts."""
    from fgnn_amd import _hip, ops
    nin, nou, net, N, M, k = q['shape']
    xd, idxd, etd = _operands(q, dev, layout)
    xd, etd = xd.requires_grad_(True), etd.requires_grad_(True)
    Wd, bd = q['W'].to(dev).requires_grad_(True), q['bias'].to(dev).requires_grad_(True)
    code = _hip.AGG_CODES[agg]
    _, am = ops.mpconv_forward_raw(xd.detach(), idxd, etd.detach(), q['W'].to(dev), q['bias'].to(dev), nou, net, 0, code, want_argmax=True)
    z = ops.mpconv(xd, idxd, etd, Wd, bd, nou, net, 0, code)
    fwd = _hip.lib().fgnn_last_kernel().decode()
    z.backward(q['gz'].to(dev)[:, :, None, :].permute(0, 3, 1, 2))
    bwd = _hip.lib().fgnn_last_kernel().decode()
    nat = lambda t: t.detach().cpu()[:, :, :, 0].permute(0, 2, 1)
    return (nat(z).float(), None if am is None else nat(am).long(), nat(xd.grad).float(), etd.grad.float().cpu().permute(0, 2, 3, 1),
            Wd.grad.cpu(), bd.grad.cpu(), fwd, bwd)


def oracle_autograd(q, agg):
    """The oracle's own autograd (f32) on the case's bf16-rounded operands: (z, gx, getype, gW, gbias) in this module's layouts."""
    import fgnn_oracle as O
    nin, nou, net, N, M, k = q['shape']
    B = q['B']
    xo = q['x'].float().permute(0, 2, 1)[:, :, :, None].contiguous().requires_grad_(True)
    eo = q['et'].float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    sd = {'filters': q['W'].clone().requires_grad_(True), 'bias': q['bias'].clone().requires_grad_(True)}
    zo = O.mp_conv(sd, '', xo, q['idx'].expand(B, -1, -1).contiguous(), eo, nou=nou, net=net, extension=0, aggregator=agg, relu=False)
    zo.backward(q['gz'].float().permute(0, 2, 1)[:, :, :, None])
    return (zo.detach()[:, :, :, 0].permute(0, 2, 1), xo.grad[:, :, :, 0].permute(0, 2, 1), eo.grad.permute(0, 2, 3, 1),
            sd['filters'].grad, sd['bias'].grad)
