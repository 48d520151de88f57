"""What the LDPC decoder tests share (test_ldpc_llr_gpu.py, test_ldpc_osd_gpu.py, test_ldpc_nms*.py, test_ldpc_decoders*.py): the named
codes, the received words of the all-zero codeword, the per-file ``paths`` fixture's body and a stand-in model.  Seeds, SNR tables,
word counts and iteration counts stay in the test files, so each file's inputs are its own."""
import functools

import numpy as np
import torch

# name -> (LdpcCode constructor and its arguments, why the code is among the cases: for the LLR-domain decoders; for the reprocessing)
CODES = {
    'g12': (('gallager', 12, 3, 6, 1), 'one partly filled wave, 6 checks; matrix and syndrome bit in one word'),
    'g33': (('gallager', 33, 3, 11, 0), 'N + 1 = 34'),
    'g63': (('gallager', 63, 3, 7, 1), 'the syndrome in bit 31 of word 1'),
    'g64': (('gallager', 64, 3, 8, 1), 'the syndrome bit opens a new word'),
    'builtin': (('builtin',), '96.3.963: 96 / 48, one wave'),
    'g32': (('gallager', 32, 16, 16, 3), 'degree 16: the per-lane worst case; dense, heavily rank-deficient'),
    'g384': (('gallager', 384, 3, 6, 1), 'E = 1152: the first size the f64 decoder refuses; 128 threads'),
    'g1024': (('gallager', 1024, 4, 8, 2), 'N at the limit, E = 4096; 256 threads, > 48 KiB of LDS, an even dv\'s rank deficiency'),
}


@functools.lru_cache(maxsize=None)
def code(name):
    """The ``LdpcCode`` of a name of ``CODES``: built once, shared."""
    from fgnn_amd.ldpc_code import LdpcCode
    (maker, *args), _ = CODES[name]
    return getattr(LdpcCode, maker)(*args)


def received(code, seed, snr_db, words):
    """LLRs [words, N] f32 (read-only) of the all-zero codeword: word b sent at snr_db[0] + (snr_db[1] - snr_db[0]) b / (words - 1) dB,
    y = -gcx + z with z from numpy's seed ``seed``, llr = -2 gcx y."""
    rng = np.random.RandomState(seed)
    gcx = 10.0 ** (np.linspace(snr_db[0], snr_db[1], words)[:, None] / 20.0)
    y = (-gcx + rng.standard_normal((words, code.n_var))).astype(np.float32)
    llr = ((-2.0 * gcx).astype(np.float32) * y).astype(np.float32)
    llr.setflags(write=False)
    return llr


def make_paths():
    """The body of a file's module-scoped ``paths`` fixture: name -> the ``LdpcDataPath`` of ``code(name)`` on cuda:0, made on first
    use and kept."""
    from fgnn_amd.datapath import LdpcDataPath
    made = {}

    def get(name):
        if name not in made:
            made[name] = LdpcDataPath('cuda:0', code(name))
        return made[name]
    return get


class ZeroLogits(torch.nn.Module):
    """A stand-in model: logits 0 for every message bit (evaluate only needs a module with a parameter on the device)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, node, *rest):
        return node[:, 0, :48, 0] * self.w, None
