"""What the two trainers share (fgnn_amd/trainloop.py), on the CPU: the log window's bookkeeping, the capture fallback around a
substituted ``graph.StepGraph``, and the resume.  The trainers themselves: tests/test_ldpc_train_gpu.py, tests/test_pgm_train_gpu.py."""
import pytest
import torch


def _row(i):
    return torch.tensor([i + 0.5, 100.0 + i, -float(i)])


def test_window_returns_the_rows_since_the_previous_read_and_the_counts_as_they_stood():
    from fgnn_amd.trainloop import LogWindow
    w = LogWindow('cpu', 3, 2, 5)
    counts, ptr = w.counts, w.counts.data_ptr()
    assert w.ring.shape == (5, 3) and w.ring.dtype == torch.float32 and counts.dtype == torch.int64 and counts.tolist() == [0, 0]
    assert w.read() is None and w.pending == 0 and w.losses == []
    reads, since = [], 0
    for i in range(12):
        full = w.push(_row(i))
        counts += torch.tensor([10, i])
        assert full == (i in (4, 9))                     # the fifth row since a read fills the ring
        if full or i == 11:
            assert w.pending == i + 1 - since
            reads.append(w.read())
            since = i + 1
            assert w.counts is counts and counts.data_ptr() == ptr and counts.tolist() == [0, 0] and w.pending == 0
    want = [(range(0, 5), [50, 0 + 1 + 2 + 3 + 4]), (range(5, 10), [50, 5 + 6 + 7 + 8 + 9]), (range(10, 12), [20, 10 + 11])]
    assert len(reads) == 3
    for (rows, got_counts), (steps, want_counts) in zip(reads, want):
        assert rows == [_row(i).tolist() for i in steps] and got_counts == want_counts
    assert w.losses == [i + 0.5 for i in range(12)] and all(type(v) is float for v in w.losses)
    before = w.ring.clone()
    assert w.read() is None                              # nothing pending: nothing changes
    assert w.pending == 0 and len(w.losses) == 12 and torch.equal(w.ring, before) and counts.tolist() == [0, 0]


def test_window_of_one_column_takes_a_scalar_and_keeps_python_floats():
    """The PGM trainer's window: a 0-dim loss per step."""
    from fgnn_amd.trainloop import LogWindow
    w = LogWindow('cpu', 1, 3, 2)
    assert not w.push(torch.tensor(0.1)) and w.push(torch.tensor(0.25))
    rows, counts = w.read()
    assert rows == [[float(torch.tensor(0.1))], [0.25]] and counts == [0, 0, 0] and w.losses == [float(torch.tensor(0.1)), 0.25]


@pytest.mark.parametrize('log_every', [0, None])
def test_window_without_log_lines_is_256_steps(log_every):
    from fgnn_amd.trainloop import LogWindow
    w = LogWindow('cpu', 3, 2, log_every)
    assert w.ring.shape == (256, 3)
    assert [w.push(_row(i)) for i in range(256)] == [False] * 255 + [True]
    assert len(w.read()[0]) == 256


def test_capture_step_reports_a_failed_capture_once_and_zeroes_the_counts(monkeypatch, capsys):
    from fgnn_amd import graph, trainloop
    counts = torch.zeros(2, dtype=torch.int64)
    seen = {}

    def failing(fn, modules=None):
        seen['modules'] = modules
        fn()                                             # a warm-up run: a real step, it counts
        assert counts.tolist() == [7, 3]
        raise ValueError('no capture today')
    monkeypatch.setattr(graph, 'StepGraph', failing)
    mods = [torch.nn.Linear(2, 2)]
    assert trainloop.capture_step(lambda: counts.add_(torch.tensor([7, 3])), mods, counts, 'some_trainer') is None
    out = capsys.readouterr()
    assert out.out == '' and out.err == 'some_trainer: hipGraph capture failed (ValueError: no capture today); running eagerly\n'
    assert seen['modules'] is mods and counts.tolist() == [0, 0]


def test_capture_step_returns_the_graph_and_zeroes_the_counts(monkeypatch, capsys):
    from fgnn_amd import graph, trainloop
    counts = torch.zeros(3, dtype=torch.int64)

    class Captured:
        def __init__(self, fn, modules=None):
            fn()
            fn()
    monkeypatch.setattr(graph, 'StepGraph', Captured)
    got = trainloop.capture_step(lambda: counts.add_(1), [], counts, 'some_trainer')
    assert isinstance(got, Captured) and counts.tolist() == [0, 0, 0]
    out = capsys.readouterr()
    assert out.out == '' and out.err == ''


def test_resume_loads_adam_and_the_scheduler_and_returns_epoch_and_gcnt():
    from fgnn_amd import trainloop

    def fresh():
        p = torch.nn.Parameter(torch.ones(3))
        opt = torch.optim.Adam([p], lr=1e-2)
        return p, opt, torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: 0.5 ** x)
    p, opt, sched = fresh()
    for _ in range(3):
        p.grad = torch.ones(3)
        opt.step()
        sched.step()
    ckpt = {'optimizer_state_dict': opt.state_dict(), 'lr_sche': sched.state_dict(), 'epoch': 3, 'gcnt': 17}
    _, opt2, sched2 = fresh()
    assert trainloop.resume(ckpt, opt2, sched2) == (3, 17)
    assert sched2.last_epoch == sched.last_epoch == 3
    assert opt2.param_groups[0]['lr'] == 1e-2 * 0.5 ** 3
    state = opt2.state_dict()['state']
    assert int(state[0]['step']) == 3 and torch.equal(state[0]['exp_avg'], opt.state_dict()['state'][0]['exp_avg'])


def test_command_line_ends(tmp_path, capsys):
    import json
    from fgnn_amd import trainloop
    there = tmp_path / 'ckpt.pt'
    there.write_bytes(b'')
    assert trainloop.existing_or_none(str(there)) == str(there)
    assert trainloop.existing_or_none(str(tmp_path / 'absent.pt')) is None and trainloop.existing_or_none(None) is None
    r = {'loss': 0.5, 'acc': 0.75, 'losses': [1.0, 0.5], 'steps': 2, 'seconds': 1.234, 'checkpoint': 'c.pt', 'err_class': [[0.0, 1.0]]}
    trainloop.report(r, True)
    assert json.loads(capsys.readouterr().out) == {k: v for k, v in r.items() if k != 'losses'}
    trainloop.report(r, False)
    assert capsys.readouterr().out == 'training done: 2 steps in 1.23 s, loss = 0.5, acc = 0.75, checkpoint c.pt\n'


def test_only_cuda_device_refuses_the_cpu():
    from fgnn_amd import trainloop
    with pytest.raises(RuntimeError, match='train runs on a ROCm device \\(no CPU fallback\\)'):
        trainloop.cuda_device('cpu')
    assert trainloop.cuda_device('cuda:1') == torch.device('cuda', 1)
