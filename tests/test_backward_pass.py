"""CPU: the host-side bookkeeping of the hand-written backwards — the parameter-gradient accumulators
(backward_pass.ParamGrads), the weight-gradient job entry point outside a backward pass, and the verdicts remembered on
the tensor that owns the memory (verdicts.remembered through ops.is_identity_list / ops._check_index_range)."""
import pytest
import torch


def _conv_with_bucket(bias=True):
    from fgnn_amd.dp import FlatGradBucket
    conv = torch.nn.Conv2d(3, 2, 1, bias=bias)
    return conv, FlatGradBucket(conv.parameters())


def test_param_grads_hands_out_the_sink_or_a_zero_accumulator():
    from fgnn_amd import ops
    conv, bucket = _conv_with_bucket()
    bare = torch.nn.Conv2d(3, 2, 1)
    bare.weight.grad = torch.ones_like(bare.weight)         # a leftover dense .grad of a parameter that never opted in
    g = ops.param_grads(torch.device('cpu'))
    assert g.acc('W', conv.weight, (2, 3, 1, 1)) is conv.weight.grad
    assert g.acc('b', conv.bias, (2,)) is conv.bias.grad
    z = g.acc('W0', bare.weight, (2, 3))
    assert z is not bare.weight.grad and z.shape == (2, 3) and z.dtype == torch.float32 and not z.any()
    assert g.acc('none', None, (2,)) is None                # no bias: no accumulator, and nothing that is not sunk
    assert g.all_sunk('W', 'b') and g.all_sunk('W', 'none') and g.all_sunk('none')
    assert not g.all_sunk('W', 'W0') and not g.all_sunk('W0')
    assert g.result('W') is None and g.result('b', torch.float32) is None and g.result('none', torch.float32) is None
    assert conv.weight.grad.data_ptr() == bucket.flat.data_ptr()


def test_param_grads_resolves_a_conv_weight_viewed_as_a_matrix():
    """A [cout, cin, 1, 1] Conv2d weight reaches the node-wise maps as its [cout, cin] view: ``.grad`` lives on the base."""
    from fgnn_amd import ops
    conv, _ = _conv_with_bucket()
    view = conv.weight.view(2, 3)
    assert view._base is conv.weight and ops.grad_sink(view) is None
    g = ops.param_grads(torch.device('cpu'))
    assert g.acc('W', view, (2, 3)) is conv.weight.grad and g.all_sunk('W') and g.result('W', view.dtype) is None
    # a view of PART of a larger tensor is not that tensor's parameter: its own accumulator
    part = conv.weight[:1]
    assert part._base is conv.weight
    z = g.acc('part', part, (1, 3, 1, 1))
    assert z is not conv.weight.grad and not g.all_sunk('part') and g.result('part').shape == part.shape
    # opted out again: the base is resolved, the sink refused
    ops.enable_grad_sink([conv.weight], False)
    assert g.acc('W', view, (2, 3)) is not conv.weight.grad and not g.all_sunk('W')


def test_param_grads_results_are_viewed_and_cast_as_asked():
    from fgnn_amd import ops
    conv = torch.nn.Conv2d(3, 2, 1).to(torch.bfloat16)      # no sink anywhere: every gradient goes back to autograd
    view = conv.weight.view(2, 3)
    g = ops.param_grads(torch.device('cpu'))
    gW = g.acc('W', view, (2, 3))
    gW4 = g.acc('W4', conv.weight, (2, 3))                  # the kernel writes [cout, cin]; the parameter is [cout, cin, 1, 1]
    gb = g.acc('b', conv.bias, (2,))
    gW.fill_(1.5), gW4.fill_(2.5), gb.fill_(3.5)
    assert g.result('W') is gW and g.result('b') is gb      # no cast asked for: the f32 accumulator itself
    r = g.result('W', view.dtype)
    assert r.dtype == torch.bfloat16 and r.shape == (2, 3) and (r == 1.5).all()
    r4 = g.result('W4', conv.weight.dtype)
    assert r4.dtype == torch.bfloat16 and r4.shape == (2, 3, 1, 1) and (r4 == 2.5).all()
    r4f = g.result('W4')
    assert r4f.dtype == torch.float32 and r4f.shape == (2, 3, 1, 1) and r4f.data_ptr() == gW4.data_ptr()
    assert g.result('b', torch.bfloat16).dtype == torch.bfloat16


def test_param_grads_follows_the_master_switch(monkeypatch):
    from fgnn_amd import ops
    conv, _ = _conv_with_bucket()
    monkeypatch.setattr(ops, 'ACCUMULATE_INTO_GRAD', False)
    g = ops.param_grads(torch.device('cpu'))
    assert g.acc('W', conv.weight, (2, 3, 1, 1)) is not conv.weight.grad and not g.all_sunk('W')


@pytest.mark.parametrize('sunk', [False, True])
def test_a_weight_gradient_job_outside_a_backward_pass_runs_at_once_and_records_nothing(sunk):
    from fgnn_amd import backward_pass
    seen = []
    backward_pass.run_wgrad(lambda record: seen.append(record), (), sunk)
    assert seen == [False] and not backward_pass.PASS.parked() and backward_pass.PASS.folds_kept() == 0


def test_identity_list_verdict_is_remembered_on_the_base_per_version_and_view(monkeypatch):
    from fgnn_amd import ops
    calls = []
    real = torch.arange
    monkeypatch.setattr(torch, 'arange', lambda *a, **k: (calls.append(1), real(*a, **k))[1])   # one call per device check
    table = real(6).reshape(1, 1, 6).repeat(2, 1, 1)        # [2, 1, 6]: two identity lists
    a = table[:1].expand(4, -1, -1)
    assert a._base is table
    assert ops.is_identity_list(a) and len(calls) == 1
    assert ops.is_identity_list(a) and ops.is_identity_list(table[:1].expand(4, -1, -1)) and len(calls) == 1      # hits
    assert getattr(table, '_fgnn_identity_list')[1] is True and not hasattr(a, '_fgnn_identity_list')             # kept on the base
    b = table[1:].expand(4, -1, -1)                         # another view of the same base (another storage offset): a miss
    assert ops.is_identity_list(b) and len(calls) == 2
    assert ops.is_identity_list(a) and len(calls) == 3      # (one verdict per tensor: the other view's replaced it)
    table[0, 0, 0] = 5                                      # the version moved: a miss, and the new answer
    assert not ops.is_identity_list(a) and len(calls) == 4
    assert not ops.is_identity_list(a) and len(calls) == 4
    assert ops.is_identity_list(b) and len(calls) == 5
    own = real(3).reshape(1, 1, 3).clone()                          # a tensor that is its own base
    assert ops.is_identity_list(own) and getattr(own, '_fgnn_identity_list')[1] is True


def test_index_range_verdict_keys_on_the_node_count(monkeypatch):
    from fgnn_amd import ops
    calls = []
    real = torch.aminmax
    monkeypatch.setattr(torch, 'aminmax', lambda t: (calls.append(1), real(t))[1])
    idx = torch.tensor([[[0, 3], [2, 1]]])
    ops._check_index_range(idx, 4)
    ops._check_index_range(idx, 4)
    assert len(calls) == 1                                  # hit
    with pytest.raises(IndexError, match=r'\[0, 3\] but x has 3 nodes'):
        ops._check_index_range(idx, 3)                      # changed extras: a miss
    assert len(calls) == 2
    with pytest.raises(IndexError):
        ops._check_index_range(idx, 3)                      # ... remembered too: it raises from the memo
    assert len(calls) == 2
    idx[0, 0, 0] = -1                                       # version bump
    with pytest.raises(IndexError, match=r'\[-1, 3\]'):
        ops._check_index_range(idx, 4)
    assert len(calls) == 3
    view = idx[:, 1:]                                       # a view: remembered on the base
    ops._check_index_range(view, 4)
    assert len(calls) == 4 and not hasattr(view, '_fgnn_index_range') and getattr(idx, '_fgnn_index_range')[1] == (1, 2)
    ops._check_index_range(torch.empty((1, 0, 2), dtype=torch.int64), 4)     # nothing to reduce
    assert len(calls) == 4


def test_verdicts_are_noted_per_site_for_a_later_capture():
    from fgnn_amd import ops, verdicts
    assert ops.Verdicts is verdicts.Verdicts
    t = torch.arange(4).reshape(1, 1, 4)
    with verdicts.Verdicts.recording() as rec:
        assert ops.is_identity_list(t)
        assert ops.is_identity_list(t)                      # a hit is not a check: noted once
        ops._check_index_range(t, 4)                        # no site: never noted
    assert list(rec.fifo) == ['identity_list'] and [v for _, v in rec.fifo['identity_list']] == [True]
    with rec.replaying():
        assert verdicts.Verdicts.recall('identity_list', t.float()) is None          # another geometry / dtype: refused
        assert verdicts.Verdicts.recall('identity_list', t) is True and rec.taken == 1
        assert verdicts.Verdicts.recall('identity_list', t) is None
