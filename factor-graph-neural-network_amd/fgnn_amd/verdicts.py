"""Host-side verdicts about device tensors (is this table shared by the batch?  an identity list?  its in-degree?): remembered on
the tensor that owns the memory (``remembered``) and carried from an eager run into a hipGraph capture of it (``Verdicts``)."""
import torch


class Verdicts:
    """The host-side verdicts of one forward (is this table shared by the batch?  an identity list?  its in-degree?  are these
    edge weights equal over the nodes?) in call order, so that a hipGraph capture of the SAME forward can take the fast paths for
    tensors it meets for the first time — tensors the model builds inside its forward (the reference's
    ``self.hnn_idx_f2v.repeat(bsize, 1, 1)``, /root/reference/train_ldpc.py:77-84) — where no host read is possible.

    ``with Verdicts.recording() as v:`` around an EAGER run notes every device check + host read; ``with v.replaying():`` around the
    capture hands them back in the same order, each only to a tensor of the same site, shape, strides and dtype (anything else:
    the conservative answer, as before).  Sound when the capture runs the same module on the same inputs in the same state — the
    tensors checked are functions of the integer inputs and of frozen parameters only; fastpath.GraphedForward re-validates both
    before every replay."""
    current = None

    def __init__(self):
        self.fifo = {}
        self.mode = None
        self.taken = 0          # verdicts handed to a capture

    @staticmethod
    def _sig(t):
        return (tuple(t.shape), tuple(t.stride()), t.dtype)

    @classmethod
    def note(cls, site, t, value):
        v = cls.current
        if v is not None and v.mode == 'record':
            v.fifo.setdefault(site, []).append((cls._sig(t), value))
        return value

    @classmethod
    def recall(cls, site, t):
        """The recorded verdict for the next check at ``site`` (None: nothing recorded / another tensor geometry)."""
        v = cls.current
        if v is None or v.mode != 'replay':
            return None
        q = v.fifo.get(site)
        if not q or q[0][0] != cls._sig(t):
            return None
        v.taken += 1
        return q.pop(0)[1]

    class _Mode:
        def __init__(self, v, mode):
            self.v, self.mode = v, mode

        def __enter__(self):
            self.prev = Verdicts.current
            self.v.mode = self.mode
            Verdicts.current = self.v
            return self.v

        def __exit__(self, *exc):
            Verdicts.current = self.prev
            self.v.mode = None
            return False

    @classmethod
    def recording(cls):
        return cls._Mode(cls(), 'record')

    def replaying(self):
        return Verdicts._Mode(self, 'replay')


_COMPUTES = object()


def remembered(t, attr, extra_key, compute, *, site=None, during_capture=_COMPUTES):
    """``compute()`` — a device check + host read about ``t`` — once per distinct tensor: the answer is remembered in attribute
    ``attr`` ON the tensor that owns the memory (the view's base, e.g. LDPCModel's frozen `hnn_idx_v2f` behind its per-call
    `expand`), keyed by version, view geometry and ``extra_key`` (where the view starts — ``data_ptr()`` or ``storage_offset()`` —
    and whatever else the answer depends on), so it can never outlive or be confused with another tensor's.

    ``during_capture``: while a hipGraph is being captured no host read is possible; an unseen tensor then gets this conservative
    answer, which is not remembered — unless an eager run of the same forward recorded its verdict for ``site`` (``Verdicts``).
    Without ``during_capture`` ``compute`` runs in a capture too.  Eager verdicts of a ``site`` are noted for such a replay."""
    owner = t._base if t._base is not None else t
    key = (t._version, tuple(t.shape), tuple(t.stride())) + tuple(extra_key)
    memo = getattr(owner, attr, None)
    if memo is not None and memo[0] == key:
        return memo[1]
    if during_capture is not _COMPUTES and t.is_cuda and torch.cuda.is_current_stream_capturing():
        value = Verdicts.recall(site, t) if site is not None else None
        if value is None:
            return during_capture
    else:
        value = compute()
        if site is not None:
            Verdicts.note(site, t, value)
    setattr(owner, attr, (key, value))
    return value
