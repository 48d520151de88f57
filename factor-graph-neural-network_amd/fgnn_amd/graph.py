"""hipGraph capture of a launch-bound step.

One LDPCModel training step is ~1500 kernel launches of 5-250 us each; at the reference batch sizes the
Python / HIP launch path (~20 us per launch) costs as much as the kernels themselves.  ``StepGraph`` records
the step once on a capture stream (every kernel of this package launches on torch's current stream, so the
hand-written HIP kernels, rocBLAS GEMMs and ATen elementwise ops all land in the same graph) and replays it
with a single launch.  Requirements are torch.cuda.graphs' usual ones: static input tensors (copy new data
into them), no host synchronisation inside the step, and no collectives (keep the gradient all-reduce outside).

One procedure (``StepGraph``; ``fastpath.GraphedForward`` from the same pieces): ``warm_up`` inside ``preserved_buffers`` (the
runs are real steps), make the weight casts stale so their refresh is recorded, capture, ``state_moved`` after every replay.
"""
import contextlib
import os

import torch

from . import _hip, ops
from .mpnn import pointwise


def state_moved():
    """Parameters / BatchNorm buffers changed behind torch's version counters (a replay, a flat optimizer): what eager code
    derived from them and cached — folded BatchNorm constants, low-precision weight copies — is stale."""
    pointwise.note_state_change()
    pointwise.invalidate_casts()


@contextlib.contextmanager
def preserved_buffers(modules):
    """Every buffer of the modules in this list (``num_batches_tracked`` and other integer buffers included) leaves the block
    with the value it entered with, also when the block raises."""
    saved = [(b, b.detach().clone()) for m in modules for b in m.buffers()]
    try:
        yield
    finally:
        for b, old in saved:
            b.copy_(old)


def warm_up(fn, n, stream):
    """``fn()`` ``n`` times on ``stream`` (allocator / workspace / autotune warm-up), then join and synchronise; returns the last
    run's value.  ``stream`` must be the capture's: autograd runs a leaf's gradient accumulation on the stream the leaf was first
    used on; after a warm-up elsewhere, parameters whose gradients come through autograd (plain torch modules such as the edge
    models of train_syn_*.py, not this package's gradient-sink kernels) would be accumulated on a branch of the graph while the
    allocator, which only knows the capture stream, hands the incoming gradient's memory to the next kernel: replayed steps
    then add garbage into those gradients (tools/diag_graph.py)."""
    dev, out = stream.device, None
    stream.wait_stream(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.stream(stream):
            for _ in range(n):
                out = fn()
    finally:                    # (also when a run raises: whoever cleans up next does so on the current stream)
        torch.cuda.current_stream(dev).wait_stream(stream)
        torch.cuda.synchronize(dev)
    return out


class StepGraph:
    def __init__(self, fn, warmup=2, static_params=False, modules=None):
        """``static_params=True`` (inference of a frozen model): the parameter-derived tensors — folded BatchNorm affines, bf16
        weight copies — are the ones the warm-up runs left in their caches, and the graph holds no kernels that rebuild them
        (the LDPC inference forward otherwise replays ~260 tiny fold / cast / copy kernels per step beside ~60 real ones).
        Replays then do NOT see parameter changes made after the capture: build a new StepGraph after loading other weights.
        Default (False): the caches are invalidated before the capture, so the refresh kernels are recorded and every replay
        derives them from the parameters as they are at that moment (what a training step needs).

        ``fn()`` is run ``warmup`` times, then captured — both on ONE side stream (``warm_up``).  With ``modules`` the first
        replay starts from the buffers the caller had (``preserved_buffers``); without, they stay advanced by the warm-up."""
        self.stream = torch.cuda.Stream()
        with preserved_buffers(() if modules is None else modules):
            warm_up(fn, warmup, self.stream)
        self.static_params = bool(static_params)
        if not self.static_params:
            pointwise.invalidate_casts()        # stale copies are refreshed in place: the capture records the refresh kernels
        self.graph = torch.cuda.CUDAGraph()
        dot = os.environ.get('FGNN_GRAPH_DOT')          # diagnosis: the captured graph (nodes, edges) as hipGraphDebugDotPrint writes it
        if dot:
            self.graph.enable_debug_mode()
        if os.environ.get('FGNN_STAMPS'):               # diagnosis: device timestamps inside the replayed step (ops.stamp)
            ops.STAMPS = {'buf': torch.zeros(8192, dtype=torch.int64, device='cuda'), 'tags': []}
        delay_ms = float(os.environ.get('FGNN_STEP_HEAD_START_MS', '0'))     # diagnosis (profiled runs): see fgnn_spin
        with torch.cuda.graph(self.graph, stream=self.stream):
            if delay_ms > 0:
                _hip.call('fgnn_spin', int(delay_ms * 1e5))
            ops.stamp('step begin')
            fn()
            ops.stamp('step end')
        self.stamps, ops.STAMPS = ops.STAMPS, None
        if dot:
            self.graph.debug_dump(dot)

    def replay(self):
        self.graph.replay()
        if not self.static_params:
            state_moved()

    def stamp_report(self, file):
        """The stamps of the LAST replay, sorted by device time (microseconds from 'step begin')."""
        if not self.stamps:
            return
        torch.cuda.synchronize()
        v = self.stamps['buf'][:len(self.stamps['tags'])].cpu().tolist()
        t0 = v[0]
        for t, tag in sorted(zip(v, self.stamps['tags'])):
            print('stamp %10.2f us  %s' % ((t - t0) / 100.0, tag), file=file)

    __call__ = replay
