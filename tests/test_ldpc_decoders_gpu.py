"""GPU: the decoders of one ``LdpcDataPath`` share one set of device tables (fgnn_amd/ldpc_decoders.py), and ``evaluate``'s
``baseline=True`` is the 'mackay' decoder spec."""
import numpy as np
import pytest
import torch

from ldpc_decoder_cases import ZeroLogits, code, received

pytestmark = pytest.mark.gpu


def test_one_path_uploads_its_tables_once(monkeypatch):
    """gallager(12, 3, 6, 1) (N 12, M 6: one partly filled wave), 5 words at 1 dB: all four decoder calls on one path, in the order
    decode, flooding, layered, reprocessing, read one upload of the incidence tables; the layers are built by the layered call only;
    and each call returns, bit for bit, what a path of its own returns."""
    from fgnn_amd.datapath import LdpcDataPath
    from fgnn_amd.ldpc_code import LdpcCode
    g12 = code('g12')
    llr = torch.from_numpy(np.array(received(g12, 9000, (1.0, 1.0), 5))).cuda()         # (a copy: the words are read-only)
    bias = torch.sigmoid(-llr.double())                                     # P(bit = 1) of these LLRs
    calls = {'incidence_tables': 0, 'layers': 0}
    for name in calls:
        def counted(self, name=name, inner=getattr(LdpcCode, name)):
            calls[name] += 1
            return inner(self)
        monkeypatch.setattr(LdpcCode, name, counted)
    steps = (('decode', lambda p: p.decode(bias, loops=20, want_posteriors=True)),
             ('flooding', lambda p: p.decode_llr(llr, 'min-sum', 'flooding', max_iter=20, want_posteriors=True)),
             ('layered', lambda p: p.decode_llr(llr, 'min-sum', 'layered', max_iter=20, want_posteriors=True)),
             ('osd', lambda p: p.decode_osd(shared['layered'][3], metric=llr, order=1)))
    path, shared = LdpcDataPath('cuda:0', g12), {}
    for what, step in steps:
        assert calls['layers'] == (1 if what == 'osd' else 0), what          # no layers before the layered call
        shared[what] = step(path)
        assert calls['incidence_tables'] == 1, what
    assert calls['layers'] == 1
    for what, step in steps:
        alone = step(LdpcDataPath('cuda:0', g12))
        assert len(alone) == len(shared[what]) == (3 if what == 'osd' else 4)
        for a, b in zip(alone, shared[what]):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), what


def test_baseline_true_is_the_mackay_spec():
    """The built-in code, 2 words per class (60 words), a model of zero logits."""
    from fgnn_amd import ldpc_eval
    ts = ldpc_eval.LdpcDataPath('cuda:0').make_test_set(num=2, baseline=False)
    model = ZeroLogits().cuda()
    assert len(ts['noizy_sg']) == 60
    flag = ldpc_eval.evaluate(model, ts, baseline=True)['baseline']['err_class']
    spec = ldpc_eval.evaluate(model, ts, baseline='mackay')['baseline']['err_class']
    listed = ldpc_eval.evaluate(model, ts, baseline=['mackay'])['baselines']['mackay']['err_class']
    assert flag.shape == (5, 6) and not np.isnan(flag).any()
    assert np.array_equal(flag, spec) and np.array_equal(flag, listed)
