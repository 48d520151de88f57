"""Node-wise (1x1) maps as GEMMs on channel-fastest activations.

The reference expresses every node-wise linear map as ``Conv2d(cin, cout, 1)`` on [B,C,N,1]
tensors (base_model.py:43-90, mp_nn_residual.py:25-35).  On ROCm that lowers to MIOpen
convolution solvers that are a poor fit for H*W = N*1 "images" (rocprof, profiles/r01: they
dominate the step).  ``PointwiseConv2d`` keeps Conv2d's parameters / state_dict keys
(``weight [cout,cin,1,1]``, ``bias``) but runs the map as one rocBLAS/hipBLASLt GEMM
[B*N, cin] x [cin, cout] on the channels-last view, which is also the layout the fused message
kernel reads and writes without a transpose.  Outputs are logical [B,C,N,W] with
channels-last strides; every consumer in this package is stride-agnostic.
"""
import ctypes
import dataclasses
import weakref

import torch

from .. import _hip, ops


_CAST_CACHE = {}          # id(tensor) -> [weakref(tensor), version, epoch, low-precision copy]
_CAST_EPOCH = 0
_FLAT_MIRRORS = []        # [flat f32 buffer (weak), {dtype: mirror}, version, epoch, {id(param): version}, params (weak)]


def invalidate_casts():
    """Mark every cached low-precision copy stale (call after updating parameters through an alias that does not
    bump their version counters, e.g. a flat parameter buffer; dp.FlatAdam does).  The copies are refreshed IN
    PLACE at their next use — their storage is never replaced, because a captured hipGraph may hold its address;
    graph.StepGraph calls this right before capturing, so the refresh kernels are part of the graph and every
    replay casts the current parameters."""
    global _CAST_EPOCH
    _CAST_EPOCH += 1


_STATE_EPOCH = 0          # bumped whenever this package changes parameters / buffers behind torch's version counters


def note_state_change():
    """Kernels write BatchNorm running statistics through raw pointers and flat optimizers update parameters through
    an alias: neither bumps the tensors' version counters.  Everything derived from them and cached across calls
    (folded eval-mode BatchNorm affines, the one-kernel inference block's weights) keys on this counter as well."""
    global _STATE_EPOCH
    _STATE_EPOCH += 1


def state_epoch():
    return _STATE_EPOCH


def refresh_in_place(old, new):
    """Derived constants cached across calls (folded BatchNorm affines, the one-kernel blocks' weight images) keep their
    STORAGE when they are recomputed: an inference hipGraph captured earlier holds these addresses, so a refresh must
    land in the same memory instead of freeing it.  Returns the tuple to keep."""
    new = tuple(t.contiguous() for t in new)
    if old is not None and len(old) == len(new) and all(
            o.shape == n.shape and o.dtype == n.dtype and o.device == n.device for o, n in zip(old, new)):
        for o, n in zip(old, new):
            o.copy_(n)
        return old
    return new


def register_flat_parameters(flat, params=()):
    """``flat`` (f32) backs many parameters (dp.FlatGradBucket(flatten_params=True)): their low-precision copies
    become views of ONE mirror buffer that is refreshed by a single cast kernel per step instead of one per tensor."""
    _FLAT_MIRRORS[:] = [e for e in _FLAT_MIRRORS if e[0]() is not None]      # buffers that are gone take their mirrors along
    _FLAT_MIRRORS.append([weakref.ref(flat), {}, -1, -1, {}, [weakref.ref(q) for q in params]])


def _from_flat_mirror(t, dtype):
    for ent in _FLAT_MIRRORS:
        flat = ent[0]()
        if flat is None:
            continue
        off = t.data_ptr() - flat.data_ptr()
        if 0 <= off < flat.numel() * 4 and t.dtype == flat.dtype and t.device == flat.device and t.is_contiguous() \
                and off % 4 == 0 and off // 4 + t.numel() <= flat.numel():
            mirror = ent[1].get(dtype)
            if mirror is None:
                mirror = ent[1][dtype] = torch.empty_like(flat, dtype=dtype)
                ent[2] = -1
            if ent[2] != flat._version or ent[3] != _CAST_EPOCH or ent[4].get(id(t)) != t._version:
                for mm in ent[1].values():
                    mm.copy_(flat)                               # one kernel for every parameter of the model
                ent[2], ent[3] = flat._version, _CAST_EPOCH
                # load_state_dict writes through the parameters, not through flat: remember every version as of now
                ent[4] = {id(q()): q()._version for q in ent[5] if q() is not None}
                ent[4][id(t)] = t._version
            return mirror[off // 4: off // 4 + t.numel()].view(t.shape)
    return None


def cast_cached(t, dtype):
    """``t.to(dtype)`` remembered until ``t`` is modified in place (optimizer step, load_state_dict):
    the forward re-uses the bf16 copies of the weights instead of re-casting ~170 tensors.  A stale copy is
    refreshed in place (same storage — see invalidate_casts)."""
    if t is None or t.dtype == dtype:
        return t
    if _FLAT_MIRRORS:
        v = _from_flat_mirror(t, dtype)
        if v is not None:
            return v
    key = id(t)
    hit = _CAST_CACHE.get(key)
    if hit is not None and hit[0]() is t and hit[3].dtype == dtype and hit[3].device == t.device and hit[3].shape == t.shape:
        if hit[1] != t._version or hit[2] != _CAST_EPOCH:
            hit[3].copy_(t.detach())
            hit[1], hit[2] = t._version, _CAST_EPOCH
        return hit[3]
    out = t.detach().to(dtype)
    # the source is held weakly: when the parameter dies its entry (and the copy) goes with it
    _CAST_CACHE[key] = [weakref.ref(t, lambda _, key=key: _CAST_CACHE.pop(key, None)), t._version, _CAST_EPOCH, out]
    return out


@dataclasses.dataclass(eq=False)
class BnHandoff:
    """A training-mode BatchNorm's batch statistics on their way from the launch that produces them to the BatchNorm that uses them.
    The caller makes one per forward and hands it to both.  A producer (``hip_linear``, ``ops.mpconv_forward_raw``) given ``bn=``
    forms the statistics of its output and FINALISES the BatchNorm itself (momentum applied to the running statistics,
    num_batches_tracked + 1), then records the rows it wrote and the statistics here; the consumer asks ``batch_stats``."""
    gamma: torch.Tensor
    beta: torch.Tensor
    running_mean: torch.Tensor
    running_var: torch.Tensor
    num_batches_tracked: torch.Tensor
    momentum: float
    eps: float
    rows: torch.Tensor = dataclasses.field(default=None, init=False)      # [R, C] the producer wrote ...
    stats: torch.Tensor = dataclasses.field(default=None, init=False)     # ... and their [4, C] mean, invstd, scale, shift

    @classmethod
    def of(cls, bn):
        """The handle of a training-mode BatchNorm module the hand-written kernels can finalise themselves, else None (eval mode, no
        running statistics, cumulative momentum, ...)."""
        if bn is None or not bn.training or not bn.track_running_stats or not bn.affine or bn.momentum is None:
            return None
        if bn.weight.dtype != torch.float32 or not bn.weight.is_cuda:
            return None
        return cls(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.momentum), float(bn.eps))

    def final(self, C, device, count, population=0, running=True):
        """(stats [4, C] f32, the fgnn_bn_final that finalises into it) for statistics over ``count`` rows standing for ``population``
        rows of the reference's tensor (0 = count).  ``running=False``: scale / shift only, the running buffers and the counter stay."""
        stats = torch.empty((4, C), device=device, dtype=torch.float32)
        rm, rv, nbt = (self.running_mean, self.running_var, self.num_batches_tracked) if running else (None, None, None)
        return stats, _hip.bn_final(stats, self.gamma.detach(), self.beta.detach(), rm, rv, nbt, self.momentum, self.eps, count,
                                    population)

    def record(self, rows, stats):
        """A producer's launch just finalised the BatchNorm with ``stats`` [4, C], the batch statistics of ``rows`` [R, C]."""
        note_state_change()                 # running statistics / num_batches_tracked were just updated in place
        self.rows, self.stats = rows, stats

    def stats_for(self, rows):
        """The producer's statistics if they describe exactly ``rows``, else None."""
        if self.stats is not None and self.rows.data_ptr() == rows.data_ptr() and self.rows.shape == rows.shape:
            return self.stats
        return None

    def batch_stats(self, rows, population=0):
        """stats [4, C] of the BatchNorm over ``rows`` [R, C]: the producer's when they describe these rows, else one reducing launch
        of csrc/bnact.hip (its last workgroup finalises).  When the producer finalised but wrote other rows (the consumer normalises
        a contiguous copy) that launch forms scale / shift only: the batch is already counted."""
        stats = self.stats_for(rows)
        if stats is not None:
            return stats
        L = _hip.lib()
        R, C = rows.shape
        stats, fin = self.final(C, rows.device, R, population, running=self.stats is None)
        ws = ops._workspace(rows.device, int(L.fgnn_bn_workspace_bytes(R, C)))
        fold = ops._fold_scratch(rows.device)
        ops.timed('bn_stats (reduce + finalise)', rows.numel() * rows.element_size(), lambda: _hip.call(
            'fgnn_bn_stats', rows, R, C, _hip.dtype_code(rows), fin, ws, ws.numel() * 4, fold))
        note_state_change()
        return stats


def hip_linear(rows, weight, bias, bn=None, transposed=False):
    """``rows @ weight.T + bias`` through csrc/linear_fwd_b16.hip (bf16 rows, f32 parameters, channel counts in
    multiples of 64): one pass over rows and the output at HBM rate, no cast of the weights.  With ``bn`` (a ``BnHandoff``) the
    launch also forms the per-channel batch statistics of the output and FINALISES that BatchNorm itself (its last workgroup:
    csrc/fgnn_gridfold.h) — running statistics, num_batches_tracked, scale / shift — and records them on the handle for the
    BatchNorm that follows.  None = shape not handled."""
    if not (rows.is_cuda and rows.dtype == torch.bfloat16 and weight.dtype == torch.float32 and rows.is_contiguous()):
        return None
    R, cin = rows.shape
    cout = weight.shape[1] if transposed else weight.shape[0]      # transposed: weight is [cin, cout] (y = rows @ weight)
    # measured on MI355X (tools/lbench.py, cold tensors, R = 393 k rows): the streaming kernel beats hipBLASLt up to 128x128 maps
    # (23.7 vs 34.4 us at 64x64, 37.7 vs 45.9 at 64x128, 52.7 vs 57.6 at 128x128: the step time does not move with that last
    # one); at 64x256 / 256x64 it loses 10 us (72 vs 61) but with the statistics epilogue saves the BatchNorm's own 25 us pass
    # over the output; wider maps stay with hipBLASLt (4 TB/s there)
    if cin * cout > (16384 if bn is not None else 8192):
        return None
    L = _hip.lib()
    npart = L.fgnn_linear_forward_partials(R, cin, cout)
    if npart == 0 or (bn is not None and R < 2):
        return None
    w = weight.detach()
    if not w.is_contiguous():
        w = w.contiguous()
    b = None if bias is None else bias.detach().float().contiguous()
    y = torch.empty((R, cout), device=rows.device, dtype=rows.dtype)
    ws = fold = fin = stats = None
    if bn is not None:
        ws = ops._workspace(rows.device, int(L.fgnn_bn_workspace_bytes(R, cout)))
        fold = ops._fold_scratch(rows.device)
        stats, fin = bn.final(cout, rows.device, R)
    ops.timed('linear_fwd_b16_kernel', 2 * R * (cin + cout),
              lambda: _hip.call('fgnn_linear_forward', rows, w, b, y, R, cin, cout, ws, fin, fold, int(transposed)),
              nflops=2 * R * cin * cout)
    if bn is not None:
        bn.record(y, stats)
    return y


def node_sum(g, M):
    """[R, C] -> [R / M, C]: sum over each sample's M consecutive rows (the gradient of a per-sample row that was broadcast over the
    sample's nodes), one pass (csrc/sum_n.hip: node_sum_kernel)."""
    R, C = g.shape
    g = g.contiguous()
    out = torch.empty((R // M, C), device=g.device, dtype=g.dtype)
    rc = []
    ops.timed('node_sum_kernel', g.numel() * g.element_size(), lambda: rc.append(_hip.invoke(
        'fgnn_node_sum', g, out, R // M, M, C, _hip.dtype_code(g))))
    if rc[0] == _hip.EUNSUPPORTED:
        # channel counts outside the kernel's 16-byte chunks (C % 8 for bf16, % 4 for f32): the broadcast path is taken for any
        # width (ops.single_source_fanout), so its backward must exist for any width too — a device-side f32 sum
        return g.view(R // M, M, C).sum(1, dtype=torch.float32).to(g.dtype)
    _hip.check(rc[0])
    return out


class _RowLinear(torch.autograd.Function):
    """y = rows @ W^T + b over R = B*N rows.  Forward and grad-input are plain GEMMs (rocBLAS /
    hipBLASLt do those well); the weight / bias gradient is the tall-skinny product
    gW = gy^T rows (K = R ~ 4e5, M,N <= 256) that rocBLAS runs 40x off its streaming bound, so it goes
    to the hand-written split-rows kernel csrc/linear_wgrad.hip (f32 accumulation, one pass over
    rows and gy)."""

    @staticmethod
    def forward(ctx, rows, weight, bias, bn=None, precomputed=None, box=None):
        """``bn``: a ``BnHandoff`` — the training-mode BatchNorm behind the map, finalised by the map's own launch.
        ``precomputed``: the output, already formed by a fused kernel (blocks.iid_mapping_in): only the graph node is made.
        ``box``: the ``ops.FanBox`` of the state ``rows`` views — the backward deposits (gy, weight) there instead of forming
        ``gy @ weight`` (the fan-out's backward multiplies all its consumers' pairs in one launch)."""
        ctx.box = box
        ctx.save_for_backward(rows, weight)
        ctx.params = (weight, bias)                     # leaf tensors (ops.grad_sink)
        if precomputed is not None:
            return precomputed
        y = hip_linear(rows, weight, bias, bn)
        if y is not None:
            return y
        w = cast_cached(weight._base if weight._base is not None else weight, rows.dtype).view(weight.shape)
        b = cast_cached(bias, rows.dtype)
        return torch.nn.functional.linear(rows, w, b)

    @staticmethod
    def backward(ctx, gy):
        rows, weight = ctx.saved_tensors
        ops.backward_node_begins()
        gy = gy.contiguous()
        if gy.dtype != rows.dtype:
            gy = gy.to(rows.dtype)
        R, cin = rows.shape
        cout = weight.shape[0]
        wparam, bparam = ctx.params
        # wide maps: bf16 multiples of 64 up to 256 and f32 multiples of 4 (csrc/linear_wgrad_f32.hip) have their own kernels;
        # what is left (odd widths) goes to the library: plain returned tensors, no sink
        library = cin * cout >= 256 * 256 and not (rows.dtype == torch.bfloat16 and cin % 64 == 0 and cout % 64 == 0
                                                   and cin <= 256 and cout <= 256) and not (
            rows.dtype == torch.float32 and cin % 4 == 0 and cout % 4 == 0 and cin <= 1024 and cout <= 1024 and R >= 2048)
        sinks = False
        if not library:
            grads = ops.param_grads(rows.device)
            gw, gb = grads.acc('weight', wparam, (cout, cin)), grads.acc('bias', bparam, (cout,))
            sinks = grads.all_sunk('weight', 'bias')
        grows = None
        taken = 0
        if ctx.needs_input_grad[0] and ctx.box is not None:
            # (gy @ weight joins the state's other gradients in the fan-out's backward — and, with the parameter gradients going to
            # sinks, this map's weight gradient joins the other consumers' there too: one pass over the state's rows for all of them)
            taken = ctx.box.deposit(gy, weight, wgrad=(rows, gw, gb) if sinks else None)
        if taken:
            grows = ctx.box.placeholder(rows.shape)
        elif ctx.needs_input_grad[0]:
            grows = hip_linear(gy, weight, None, transposed=True)      # gy [R,cout] @ weight [cout,cin]
            if grows is None:
                grows = gy @ cast_cached(weight._base if weight._base is not None else weight, gy.dtype).view(weight.shape)
        if taken == 2:
            return grows, None, None, None, None, None
        if library:
            gw = (gy.t() @ rows).float()                # f32 square 256-wide maps: rocBLAS is ahead there
            gb = gy.float().sum(0) if bparam is not None else None
            return grows, gw.to(weight.dtype), (gb.to(weight.dtype) if gb is not None else None), None, None, None

        def launch(record, rows=rows, gy=gy, gw=gw, gb=gb):      # (the closure keeps rows / gy alive until the kernel is issued)
            ops.linear_wgrad(rows, [(gy, gw, gb)], record)
        grads.run_wgrad(launch, (rows, gy), 'weight', 'bias')
        return grows, grads.result('weight', weight.dtype), grads.result('bias', weight.dtype), None, None, None


class PointwiseConv2d(torch.nn.Conv2d):
    def __init__(self, in_channels, out_channels, kernel_size=1, bias=True):
        assert kernel_size in (1, (1, 1)), 'PointwiseConv2d is a 1x1 map'
        super().__init__(in_channels, out_channels, 1, bias=bias)

    def forward(self, x, bn=None):
        """``bn``: the ``BnHandoff`` of the training-mode BatchNorm the caller hands the result straight to (with the same handle).
        The map's launch then forms that BatchNorm's batch statistics in its epilogue and finalises them (running statistics
        included): the BatchNorm neither re-reads the tensor for them nor launches a finaliser."""
        B, C, H, W = x.shape
        rows = x.permute(0, 2, 3, 1)                    # [B,H,W,C] view; free when channels-last
        if not rows.is_contiguous():
            rows = rows.contiguous()
        rows = rows.view(B * H * W, C)
        if torch.is_autocast_enabled():
            rows = rows.to(torch.get_autocast_dtype('cuda'))
        weight = self.weight.view(self.out_channels, C)
        if rows.is_cuda and rows.dtype in (torch.float32, torch.bfloat16) and torch.is_grad_enabled() and (
                weight.requires_grad or rows.requires_grad):
            y = _RowLinear.apply(rows, weight, self.bias, bn, None, ops.fan_box(x))
        else:
            needs_grad = torch.is_grad_enabled() and (weight.requires_grad or rows.requires_grad)
            y = hip_linear(rows, weight, self.bias) if rows.is_cuda and not needs_grad else None
            if y is None and needs_grad:
                # dtypes / devices outside the hand-written path (f64 gradcheck, fp16 autocast, CPU bf16): a plain
                # differentiable cast — never the detached cached copies, which would train with zero weight gradients
                b = None if self.bias is None else self.bias.to(rows.dtype)
                y = torch.nn.functional.linear(rows, weight.to(rows.dtype), b)
            elif y is None:
                w = cast_cached(self.weight, rows.dtype).view(self.out_channels, C)
                b = cast_cached(self.bias, rows.dtype)
                y = torch.nn.functional.linear(rows, w, b)
        return y.view(B, H, W, self.out_channels).permute(0, 3, 1, 2)


class _InstNormAct(torch.autograd.Function):
    """act(InstanceNorm(x)) over the node axis of a channel-fastest [B,C,N,1] tensor: one HIP kernel
    forward, one backward (csrc/instnorm.hip); only x is saved."""

    @staticmethod
    def forward(ctx, x, relu, precomputed=None):
        """``precomputed``: the output rows [B,N,1,C], already formed by a fused kernel (blocks.iid_mapping_in)."""
        B, C, N, _ = x.shape
        rows = x.permute(0, 2, 3, 1)                    # [B,N,1,C]
        if not rows.is_contiguous():
            rows = rows.contiguous()
        ctx.save_for_backward(rows)
        ctx.relu = relu
        if precomputed is not None:
            return precomputed.permute(0, 3, 1, 2)
        y = torch.empty_like(rows)
        ops.timed('instnorm_fwd_kernel', 2 * rows.numel() * rows.element_size(),
                  lambda: _hip.call('fgnn_instnorm_forward', rows, y, B, N, C, _hip.dtype_code(rows), int(relu)))
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, gy):
        (rows,) = ctx.saved_tensors
        ops.backward_node_begins()
        B, N, _, C = rows.shape
        g = gy.permute(0, 2, 3, 1)
        if not g.is_contiguous() or g.dtype != rows.dtype:
            g = g.to(rows.dtype).contiguous()
        gx = torch.empty_like(rows)
        ops.timed('instnorm_bwd_kernel', 3 * rows.numel() * rows.element_size(),
                  lambda: _hip.call('fgnn_instnorm_backward', rows, g, gx, B, N, C, _hip.dtype_code(rows), int(ctx.relu)))
        return gx.permute(0, 3, 1, 2), None, None


class _InstNormDot(torch.autograd.Function):
    """out[b,0,n,0] = bias + sum_c w[c] relu(InstanceNorm(x)[b,c,n,0]) — the classifier's InstanceNorm2d -> ReLU -> Conv2d(128, 1, 1)
    (factor_mpnn_sp.py:104-108) as one kernel forward and one backward (csrc/instnorm.hip: instnorm_dot_kernel); only x is saved,
    neither the normalised tensor nor its gradient exists in memory."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        B, C, N, _ = x.shape
        rows = x.permute(0, 2, 3, 1)
        if not rows.is_contiguous():
            rows = rows.contiguous()
        w = weight.detach().reshape(C)
        out = torch.empty((B, 1, N, 1), device=x.device, dtype=x.dtype)
        ops.timed('instnorm_dot_kernel<fwd>', rows.numel() * rows.element_size(), lambda: _hip.call(
            'fgnn_instnorm_dot_forward', rows, w, None if bias is None else bias.detach(), out, B, N, C, _hip.dtype_code(rows)))
        ctx.save_for_backward(rows, weight)
        ctx.params = (weight, bias)
        return out

    @staticmethod
    def backward(ctx, gout):
        rows, weight = ctx.saved_tensors
        ops.backward_node_begins()
        B, N, _, C = rows.shape
        L = _hip.lib()
        g = gout.reshape(B, N)
        if not g.is_contiguous() or g.dtype != rows.dtype:
            g = g.to(rows.dtype).contiguous()
        wparam, bparam = ctx.params
        grads = ops.param_grads(rows.device)
        gw, gb = grads.acc('weight', wparam, wparam.shape), grads.acc('bias', bparam, (1,))
        gx = torch.empty_like(rows)
        ws = ops._workspace(rows.device, int(L.fgnn_instnorm_dot_workspace_bytes(B)))
        ops.timed('instnorm_dot_kernel<bwd>', 2 * rows.numel() * rows.element_size(), lambda: _hip.call(
            'fgnn_instnorm_dot_backward', rows, weight.detach(), g, gx, gw, gb, B, N, C, _hip.dtype_code(rows), ws, ws.numel() * 4))
        return gx.permute(0, 3, 1, 2), grads.result('weight', wparam.dtype), grads.result('bias', None if bparam is None else bparam.dtype)


INSTNORM_DOT = True       # (module switch: the classifier's closing pair staged when False)


def instnorm_relu_dot(x, conv):
    """``conv(relu(InstanceNorm2d(x)))`` for a one-output 1x1 ``conv`` over 128 channels (the classifier head's closing pair) as
    one kernel, or None when the shape / dtype / device is not the kernel's (the caller then runs the staged modules)."""
    if not (INSTNORM_DOT and x.is_cuda and x.dim() == 4 and x.shape[3] == 1 and x.shape[1] == 128 and 2 <= x.shape[2] <= 128
            and x.dtype in (torch.float32, torch.bfloat16) and isinstance(conv, torch.nn.Conv2d) and conv.out_channels == 1
            and conv.in_channels == 128 and conv.weight.dtype == torch.float32 and conv.weight.is_contiguous()
            and (conv.bias is None or conv.bias.dtype == torch.float32)):
        return None
    if torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad):
        return _InstNormDot.apply(x, conv.weight, conv.bias)
    B, C, N, _ = x.shape
    rows = x.permute(0, 2, 3, 1)
    if not rows.is_contiguous():
        rows = rows.contiguous()
    out = torch.empty((B, 1, N, 1), device=x.device, dtype=x.dtype)
    ops.timed('instnorm_dot_kernel<fwd>', rows.numel() * rows.element_size(), lambda: _hip.call(
        'fgnn_instnorm_dot_forward', rows, conv.weight.detach(), None if conv.bias is None else conv.bias.detach(), out, B, N, C,
        _hip.dtype_code(rows)))
    return out


class NodeInstanceNorm(torch.nn.Module):
    """InstanceNorm2d(affine=False, no running stats) over the node axis of [B,C,N,1], any strides,
    optionally fused with the ReLU that follows it in every reference use (``relu=True``).

    A single node (the LDPC hyper-factor, factor_mpnn_sp.py:77,140) normalises to exactly 0
    — (x-mean)/sqrt(0+eps) — which is what the reference's torch-1.0 era computed and what
    newer torch refuses to compute.  No parameters, so state_dicts match
    torch.nn.InstanceNorm2d's (empty) contribution.
    """
    eps = 1e-5

    def __init__(self, relu=False):
        super().__init__()
        self.relu = relu

    def forward(self, x):
        if x.shape[2] * x.shape[3] == 1:
            return torch.zeros_like(x)
        if x.is_cuda and x.shape[3] == 1 and x.dtype in (torch.float32, torch.bfloat16):
            return _InstNormAct.apply(x, self.relu)
        xf = x.float()                                   # statistics in f32 also for bf16 activations
        var, mean = torch.var_mean(xf, dim=(2, 3), unbiased=False, keepdim=True)
        y = ((xf - mean) * torch.rsqrt(var + self.eps)).to(x.dtype)
        return torch.relu(y) if self.relu else y


def as_addends(addend):
    """``addend`` arguments are one tensor, None, or a list of tensors / Nones: the list of tensors."""
    if addend is None:
        return []
    if isinstance(addend, (list, tuple)):
        return [a for a in addend if a is not None]
    return [addend]


def add_all(y, addend):
    for a in as_addends(addend):
        y = y + a
    return y


def split_broadcast(addends):
    """``addends`` (tensors [B, C, N, 1]) -> (tensors, periods): an addend that is a per-sample vector broadcast over the N nodes
    (``ops.broadcast_nodes``: the LDPC hyper-factor's message to the variables) is replaced by its [B, C, 1, 1] source with period N —
    the apply kernels read it as one row per N output rows and its gradient is the node sum of the output's."""
    ts, periods = [], []
    for a in addends:
        src = getattr(a, '_fgnn_bcast_src', None)
        if src is not None and a.shape[2] > 1:
            ts.append(src)
            periods.append(int(a.shape[2]))
        else:
            ts.append(a)
            periods.append(1)
    return ts, periods


def period_array(periods):
    periods = (list(periods) + [1, 1, 1])[:3]
    return None if all(q == 1 for q in periods) else (ctypes.c_int32 * 3)(*periods)


class _BatchNormAct(torch.autograd.Function):
    """Train-mode BatchNorm + LeakyReLU(slope) on channel-fastest rows [R, C] (csrc/bnact.hip)."""

    @staticmethod
    def forward(ctx, rows, weight, bias, handoff, slope, addend=None, addend2=None, addend3=None, periods=(1, 1, 1), population=0):
        """``handoff``: the BatchNorm's ``BnHandoff`` (running statistics, counter, momentum, eps; the statistics of a producer in
        front of it); ``weight`` / ``bias`` are its gamma / beta as arguments of their own, for autograd.  ``periods``: an addend
        with period m has one row per m rows of the output (a per-sample vector broadcast over the sample's m nodes).
        ``population``: rows the statistics stand for in the running variance's unbiased correction (0 = R)."""
        R, C = rows.shape
        dt = _hip.dtype_code(rows)
        stats = handoff.batch_stats(rows, population)
        y = torch.empty_like(rows)
        ctx.has_addend = tuple(a is not None for a in (addend, addend2, addend3))
        ctx.periods = tuple(periods)
        ops.timed('bn_apply (forward)', (2 + sum(ctx.has_addend)) * rows.numel() * rows.element_size(),
                  lambda: _hip.call('fgnn_bn_apply', rows, y, R, C, dt, stats[2], stats[3], slope, addend, addend2, addend3,
                                    period_array(periods)))
        ctx.save_for_backward(rows, weight, bias, stats)
        ctx.slope = slope
        ctx.params = (weight, bias)
        return y

    @staticmethod
    def backward(ctx, gy):
        ops.backward_node_begins()
        rows, weight, bias, stats = ctx.saved_tensors
        L = _hip.lib()
        R, C = rows.shape
        gy = gy.contiguous()
        if gy.dtype != rows.dtype:
            gy = gy.to(rows.dtype)
        gx = torch.empty_like(rows)
        grads = ops.param_grads(rows.device)
        gw, gb = grads.acc('gamma', ctx.params[0], (C,)), grads.acc('beta', ctx.params[1], (C,))
        ws = ops._workspace(rows.device, int(L.fgnn_bn_workspace_bytes(R, C)))
        fold = ops._fold_scratch(rows.device)
        ops.timed('bn_backward (reduce + finalise + apply)', 5 * rows.numel() * rows.element_size(),
                  lambda: _hip.call('fgnn_bn_backward', rows, gy, gx, R, C, _hip.dtype_code(rows), stats[0], stats[1], weight, bias,
                                    ctx.slope, gw, gb, ws, ws.numel() * 4, fold))
        ga = [None, None, None]
        for i in range(3):
            if ctx.has_addend[i] and ctx.needs_input_grad[5 + i]:
                ga[i] = gy if ctx.periods[i] == 1 else node_sum(gy, ctx.periods[i])
        return (gx, grads.result('gamma'), grads.result('beta'), None, None, *ga, None, None)


class BatchNormAct2d(torch.nn.BatchNorm2d):
    """``BatchNorm2d`` (same parameters / buffers / state_dict keys) that also applies the activation the
    reference puts right behind it — ``slope`` 0.01 = LeakyReLU (conv1/conv2 of mp_conv_residual), 0 = ReLU
    (iid_mapping_bn, mp_conv_v2's own bn) — in one fused HIP kernel pair when training on a ROCm device;
    everything else (eval mode, CPU, odd channel counts) goes through torch's batch_norm + activation."""

    def __init__(self, num_features, slope=0.0):
        super().__init__(num_features)
        self.slope = float(slope)

    @staticmethod
    def _activate(y, slope):
        if slope == 0.0:
            return torch.relu(y)
        if slope == 1.0:
            return y
        return torch.nn.functional.leaky_relu(y, slope)

    def forward(self, x, addend=None, slope=None, population_mult=1, handoff=None):
        """``addend`` (a tensor of the output's shape, or a list of up to three) is added AFTER the activation — the
        ``acc + block(x) (+ residual + skip)`` that follows every block in FactorNN rides in the apply kernel
        instead of being separate passes.  ``slope`` overrides the module's activation for this call (mp_conv_v2 asks its
        plain BatchNorm for the fused ReLU this way: an argument, not a toggled attribute).  ``population_mult`` = m: every row of
        ``x`` stands for m identical rows of the reference's tensor (a per-sample vector the reference broadcasts over m nodes
        before this BatchNorm): same mean and biased variance, the running variance's unbiased correction counts m times the rows.
        ``handoff``: the ``BnHandoff`` the caller gave the producer of ``x`` (``PointwiseConv2d.forward``, ``ops.mpconv``)."""
        slope = self.slope if slope is None else float(slope)
        B, C, H, W = x.shape
        addends = as_addends(addend)
        if len(addends) > 3:
            addends = addends[:2] + [ops.add_n(addends[2:])]
        # momentum=None (cumulative average) and a one-value batch in training mode (torch raises) stay with torch
        ok = (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and self.track_running_stats and
              self.affine and self.momentum is not None and (not self.training or B * H * W > 1) and
              _hip.lib().fgnn_bn_supported(B * H * W, C, _hip.dtype_code(x)))
        wants_grad = torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad or
                                                  any(a.requires_grad for a in addends))
        if not ok or (not self.training and wants_grad):
            if population_mult != 1 and self.training:
                raise _hip.FgnnHipError('BatchNormAct2d: population_mult needs the HIP path (a ROCm tensor, running statistics)')
            if self.training and handoff is not None and handoff.stats is not None:
                # the map in front already finalised this BatchNorm (momentum applied, batch counted): batch statistics only here
                y = torch.nn.functional.batch_norm(x, None, None, self.weight, self.bias, True, 0.0, self.eps)
                return add_all(self._activate(y, slope), addends)
            return add_all(self._activate(super().forward(x), slope), addends)
        rows = x.permute(0, 2, 3, 1)
        if not rows.is_contiguous():
            rows = rows.contiguous()
        rows = rows.view(B * H * W, C)
        addends, periods = split_broadcast(addends)
        arows = [None, None, None]
        for i, a in enumerate(addends):
            ar = a.permute(0, 2, 3, 1)
            if ar.dtype != rows.dtype or not ar.is_contiguous():
                ar = ar.to(rows.dtype).contiguous()
            arows[i] = ar.view(-1, C)
        periods = tuple((periods + [1, 1, 1])[:3])
        if self.training:                               # num_batches_tracked += 1 rides in the statistics finaliser
            if handoff is None:
                handoff = BnHandoff(self.weight, self.bias, self.running_mean, self.running_var, self.num_batches_tracked,
                                    self.momentum, self.eps)
            y = _BatchNormAct.apply(rows, self.weight, self.bias, handoff, slope, *arows, periods,
                                    0 if population_mult == 1 else B * H * W * population_mult)
        else:                                           # eval: folded affine + activation in one pass
            scale, shift = self._folded()
            y = torch.empty_like(rows)
            _hip.call('fgnn_bn_apply', rows, y, B * H * W, C, _hip.dtype_code(rows), scale, shift, slope, *arows, period_array(periods))
        return y.view(B, H, W, C).permute(0, 3, 1, 2)

    def _folded(self):
        """Eval-mode BatchNorm as (scale, shift); recomputed only when a parameter / buffer changed."""
        key = (self.weight._version, self.bias._version, self.running_mean._version, self.running_var._version,
               self.weight.device, state_epoch())
        if getattr(self, '_fold_key', None) != key:
            with torch.no_grad():
                scale = self.weight.float() * torch.rsqrt(self.running_var.float() + self.eps)
                shift = self.bias.float() - self.running_mean.float() * scale
            self._fold_key = key
            self._fold = refresh_in_place(getattr(self, '_fold', None), (scale, shift))
        return self._fold
