"""Host-side bookkeeping of a backward pass: where parameter gradients accumulate (``ParamGrads``) and when the launches that
produce them go out (``BackwardPass``, one per process: ``PASS``).  Imports neither ``ops`` nor ``mpnn``: every hand-written
backward can import it at module top.
"""
import torch

from . import _hip


# ---- deferred weight-gradient kernels -------------------------------------------------------------------------------------
# Nothing in a backward pass READS a weight gradient: the kernels that produce them (2.6 ms of a 18.8 ms LDPC step) only have to be
# done before the optimizer.  FactorNN's two streams spend the backward waiting for each other at every layer's joins (the
# main stream 3.5 ms, the side stream 7 ms of a step: profiles/r03/train_step_timeline.txt), so a weight-gradient kernel that sits
# in stream order IN FRONT of a kernel the other stream waits for is on the critical path for nothing.  With DEFER_WGRAD the
# launches are parked per stream and issued when the autograd engine moves on to a node of ANOTHER stream — i.e. right behind the
# stream's last critical kernel, into the slot where it would otherwise idle until the join — and at the latest when the
# backward pass ends (an engine callback, which also joins every such stream into the caller's).  Only gradients that go to
# a sink (ops.grad_sink: the flat bucket) are deferred: a gradient tensor handed back to autograd must be complete in stream order.
DEFER_WGRAD = True          # (module switch: tests compare parked against inline launches)
# (round 5 also tried the parked launches on a THIRD stream and on the side stream, each behind an event on its operands: 15.5 / 15.1
#  against 13.8 ms — every kernel that overlaps an operator launch waits for a CU; profiles/r05/README.md.  Removed.)

# ---- recorded parameter-gradient folds -------------------------------------------------------------------------------------------
# Every weight / filter gradient kernel leaves per-workgroup slabs that a small launch folds into the accumulator: ~100 launches of
# 5-15 us per LDPC step, a third of them in the main stream's dependent chain (csrc/fold_batch.hip).  When the gradient goes to a
# sink (ops.grad_sink: nothing in the pass reads it) the fold is RECORDED instead — the call gets a slab buffer of its own, kept
# alive here — and ONE launch at the end of the pass folds them all (a fixed summation order of its own: reproducible, equal to the
# immediate folds' sums to f32 rounding).
DEFER_FOLDS = True          # (module switch: tests compare recorded against immediate folds)

TAIL_TO_SIDE = True         # see BackwardPass.tail_begins (module switch for the A/B in tools/ and the tests)


class _FoldScope:
    """``with PASS.fold_scope(defer, scratch):`` — the gradient entry points called inside record their slab folds
    (csrc/fold_batch.hip) when ``defer``; ``slabs(device, nbytes)`` is the workspace to hand them: a private buffer (alive until
    the flush) then, else ``scratch(device, nbytes)``, the stream's shared one."""

    def __init__(self, keep, defer, scratch):
        self.keep, self.defer, self.scratch = keep, bool(defer), scratch

    def slabs(self, device, nbytes):
        if not self.defer:
            return self.scratch(device, nbytes)
        t = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
        self.keep.append(t)
        return t

    def __enter__(self):
        if self.defer:
            _hip.lib().fgnn_fold_defer(1)
        return self

    def __exit__(self, *exc):
        if self.defer:
            _hip.lib().fgnn_fold_defer(0)
        return False


class BackwardPass:
    """What the hand-written backwards of ONE autograd pass leave for later: parked weight-gradient launches and recorded folds."""

    def __init__(self):
        self.side_active = False    # set by the assemblies the first time a forward actually forks onto the side stream: with ONE stream in
                                    # play parking buys no overlap and only keeps every layer's operands alive until the end of the backward
        self._parked = {}           # stream -> [(launch closure, operands)]
        self._task = None           # id of the backward pass (autograd graph task) whose end-of-pass callback is queued
        self._issued = set()        # streams that got parked launches issued during the current backward pass
        self._fold_keep = []        # slab buffers of the recorded folds

    def park(self, launch, operands=()):
        """Park `launch` (a closure that enqueues one weight-gradient kernel on the CURRENT stream).  `operands`: the tensors the
        kernel reads.  They are kept alive until the kernel is issued and then marked as in use by its stream: an activation the
        OTHER stream allocated is otherwise handed back to that stream's allocator the moment the last reference drops — the
        engine's join with this stream happened before the parked kernel went out, so nothing else orders the reuse behind it
        (found as three weight gradients of hyper-factor maps reading overwritten rows on hipGraph replay)."""
        if not DEFER_WGRAD or not self.side_active:
            launch()
            return
        st = torch.cuda.current_stream()
        task = torch._C._current_graph_task_id()           # (-1 outside a backward pass: then nothing would ever issue the launch)
        if task < 0:
            launch()
            return
        self._enter(task)
        self._parked.setdefault(st, []).append((launch, tuple(operands)))

    def _enter(self, task):
        if self._task != task:
            # Another backward pass than the one that parked what is in the lists: a NESTED (re-entrant) pass inside it — checkpointing,
            # a custom Function calling backward() — or a pass that died half-way.  Either way the parked launches are ISSUED, never
            # dropped (they accumulate into sinked .grad buffers behind autograd's back: dropping them would lose gradients silently;
            # issuing those of a dead pass only finishes an accumulation its owner discards).  The outer pass re-registers itself
            # with its next parked launch; its own end-of-pass callback is still queued.
            if self.parked():
                self._issue_parked()
            self.flush_folds()
            self._task = task
            torch.autograd.Variable._execution_engine.queue_callback(self._end_of_pass)

    def parked(self):
        """Is any launch parked?"""
        return any(self._parked.values())

    def folds_kept(self):
        """Number of slab buffers kept for recorded folds that were not flushed yet."""
        return len(self._fold_keep)

    def folds_deferrable(self):
        """True inside a backward pass whose end this object gets to see (the engine callback that flushes the recorded folds)."""
        if not DEFER_FOLDS:
            return False
        task = torch._C._current_graph_task_id()
        if task < 0:
            return False
        self._enter(task)
        return True

    def fold_scope(self, defer, scratch):
        return _FoldScope(self._fold_keep, defer, scratch)

    def flush_folds(self):
        """Fold everything recorded, on the current stream (the caller has ordered it behind every producer)."""
        L = _hip.lib()
        if L.fgnn_fold_pending():
            _hip.call('fgnn_fold_flush')
            cur = torch.cuda.current_stream()
            for t in self._fold_keep:       # slabs another stream allocated are read by this stream's launch: not that stream's to reuse yet
                t.record_stream(cur)
        self._fold_keep.clear()

    def _issue(self, lst, st):
        """Issue the parked launches ``lst`` on stream ``st`` (the current one)."""
        for fn, operands in lst:
            fn()
            for t in operands:
                t.record_stream(st)
        lst.clear()
        self._issued.add(st)

    def _issue_parked(self, except_stream=None):
        """Issue the parked launches of every stream but `except_stream`, each on its own stream."""
        for st, lst in self._parked.items():
            if lst and (except_stream is None or st != except_stream):
                with torch.cuda.stream(st):
                    self._issue(lst, st)

    def drain(self):
        """Issue whatever is parked, join the streams it was issued on into the current one and fold what was recorded."""
        self._issue_parked()
        cur = torch.cuda.current_stream()
        for st in self._issued:     # the engine joined its streams BEFORE its callback (never, for a pass that died): what was issued since needs its own join
            if st != cur:
                cur.wait_stream(st)
        self.flush_folds()          # every producer is now in front of the current stream: one launch folds all their slabs
        self._issued.clear()

    def _end_of_pass(self):
        self._task = None
        self.drain()

    def _in_registered_pass(self):
        return self._task is not None and self._task == torch._C._current_graph_task_id()

    def node_begins(self):
        """Called at the top of every hand-written backward: the engine has moved to a node on the current stream, so the other
        streams' parked weight-gradient launches go out now (behind their last critical kernel)."""
        if self._in_registered_pass():
            self._issue_parked(except_stream=torch.cuda.current_stream())

    def tail_begins(self, side_stream):
        """Called by a backward node behind which the pass is ONE dependent chain on the current stream — the edge-type MLPs' backward,
        which needs the edge-weight gradients of all eight layers (/root/reference/train_ldpc.py:68-69: `emodel_*` feed every layer).
        What is parked for the end of the pass — this stream's weight-gradient launches and every recorded parameter-gradient fold —
        used to run BEHIND that chain, alone on the chip (0.3 ms of a 13 ms step: profiles/r06/README.md); it goes to the side stream
        (``side_stream(device)``) NOW, behind an event on this stream, and runs beside the chain.  The end-of-pass callback joins the
        side stream as before."""
        if not (TAIL_TO_SIDE and self.side_active and self._in_registered_pass()):
            return
        cur = torch.cuda.current_stream()
        side = side_stream(cur.device)
        if side == cur:
            return
        self._issue_parked(except_stream=cur)        # (the other streams' parked launches go out on their own streams, as at any node)
        mine = self._parked.get(cur) or []
        if not mine and not _hip.lib().fgnn_fold_pending():
            return
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            self._issue(mine, side)
            self.flush_folds()      # every producer recorded so far is in front of `ready` on this stream or earlier on the side stream


PASS = BackwardPass()


def run_wgrad(launch, operands, sunk):
    """Run one weight-gradient job: ``launch(record)`` enqueues its kernel(s) on the current stream, ``record`` telling
    ``ops.linear_wgrad`` to record the slab folds.  With every parameter gradient of the job going to a sink (``sunk``) nothing in
    the backward reads the result: the launch is parked and issued where its stream would otherwise wait for the other one
    (``BackwardPass.park``).  ``record`` is decided here, inside the pass: a parked launch may go out from its end-of-pass callback."""
    record = sunk and PASS.folds_deferrable()
    if sunk:
        PASS.park(lambda: launch(record), operands)
    else:
        launch(record)


class ParamGrads:
    """The f32 accumulators the gradient kernels of one backward node add into, one per parameter: ``param.grad`` itself where
    ``sink(param)`` hands it out (``ops.grad_sink``: autograd then gets None for that input), else a zero tensor that is
    returned to autograd."""

    def __init__(self, device, sink):
        self.device, self.sink = device, sink
        self._entries = {}      # name -> (parameter as the Function got it, accumulator, sunk)

    def acc(self, name, param, shape):
        """The accumulator for ``param`` — the leaf as saved in ``ctx.params`` — in the ``shape`` the kernel writes.  A
        [cout, cin, 1, 1] Conv2d parameter viewed as [cout, cin] has its ``.grad`` on the base.  None (no bias) -> None, sunk."""
        if param is None:
            self._entries[name] = (None, None, True)
            return None
        owner = param._base if param._base is not None and param._base.numel() == param.numel() else param
        g = self.sink(owner)
        sunk = g is not None
        if not sunk:
            g = torch.zeros(shape, device=self.device, dtype=torch.float32)
        self._entries[name] = (param, g, sunk)
        return g

    def all_sunk(self, *names):
        return all(self._entries[n][2] for n in names)

    def run_wgrad(self, launch, operands, *names):
        """``run_wgrad`` for a job whose parameters are ``names``."""
        run_wgrad(launch, operands, self.all_sunk(*names))

    def result(self, name, dtype=None):
        """What autograd gets for the parameter: None when its gradient went to the sink (or there is no such parameter), else
        the accumulator in the parameter's shape, cast to ``dtype`` if one is given."""
        param, g, sunk = self._entries[name]
        if sunk:
            return None
        if g.shape != param.shape:
            g = g.view(param.shape)
        return g if dtype is None else g.to(dtype)
