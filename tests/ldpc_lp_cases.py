"""What the ADMM-LP decoder tests share (test_ldpc_lp.py on the CPU, test_ldpc_lp_gpu.py on the device): the codes and received words,
the decoder settings of every comparison, the restatement's cached results, and the brute-force maximum-likelihood check of the ML
certificate.  Nothing here touches a device.

Inputs: the codes of ldpc_decoder_cases.CODES named in ``CODES`` at test_ldpc_llr_gpu.py's ``SNR_DB``, 67 words each; 'irregular', a
hand-made matrix with a degree-2 and a degree-1 check (``LdpcCode`` refuses it, so its tables are built here and it is decoded
through the C entry point); 'g768' = gallager(768, 8, 16, 1), whose word state passes 48 KiB, with five words at 4 dB.

Fixed-count settings (``FIXED``): eps = -1 and stop_on_codeword = 0, so every word runs max_iter iterations.  (eps = 0 would not do:
a word whose iterates reach an integral fixed point has res = dz = 0 exactly and stops there, and the two precisions of the
restatement reach that point at different iterations.)"""
import functools

import numpy as np

import ldpc_llr_oracle as LO
import ldpc_lp_oracle as LP
from ldpc_decoder_cases import code as named_code, received

B = 67
CODES = ('g12', 'builtin', 'g32', 'g384', 'g1024')
SNR_DB = {'g12': (3.0, 3.0), 'builtin': (2.5, 2.5), 'g32': (3.0, 3.0), 'g384': (0.5, 6.5), 'g1024': (1.0, 7.0)}      # test_ldpc_llr_gpu.py's
# rows over 6 variables: {0,1,3}, {1,2,4}, {0,4,5}, {2,3}, {5}
IRREGULAR_NLIST = np.array([[0, 2], [0, 1], [1, 3], [0, 3], [1, 2], [2, 4]])

PLAIN = dict(mu=3.0, penalty=0.0, eps=-1.0, stop_on_codeword=0)
PENALISED = dict(mu=3.0, penalty=0.8, relax=1.9, eps=-1.0, stop_on_codeword=0)
# name -> the decoder's keyword arguments
FIXED = {'plain-r1.0-i1': dict(PLAIN, relax=1.0, max_iter=1), 'plain-r1.0-i8': dict(PLAIN, relax=1.0, max_iter=8),
         'plain-r1.0-i50': dict(PLAIN, relax=1.0, max_iter=50), 'plain-r1.9-i8': dict(PLAIN, relax=1.9, max_iter=8),
         'pen-i1': dict(PENALISED, max_iter=1), 'pen-i3': dict(PENALISED, max_iter=3), 'pen-i8': dict(PENALISED, max_iter=8)}
G1024_FIXED = ('plain-r1.0-i1', 'plain-r1.0-i8', 'plain-r1.9-i8', 'pen-i1', 'pen-i3', 'pen-i8')         # at 1 and 8 (and 3) only
STOP = {'plain-stop': dict(mu=3.0, penalty=0.0, relax=1.9, eps=1e-5, stop_on_codeword=0, max_iter=100),
        'pen-stop': dict(mu=3.0, penalty=0.8, relax=1.9, eps=1e-5, stop_on_codeword=1, max_iter=20)}
SETTINGS = dict(FIXED, **STOP)
CERTIFICATE = dict(mu=3.0, penalty=0.0, relax=1.0, eps=1e-5, stop_on_codeword=0, max_iter=300)


def fixed_cases():
    """Every (code, fixed-count setting) compared."""
    return [(name, key) for name in CODES + ('irregular', 'g768') for key in FIXED if name != 'g1024' or key in G1024_FIXED]


@functools.lru_cache(maxsize=None)
def case(name):
    """(tables, llr [B, N] f32, read-only) of one input."""
    if name == 'irregular':
        llr = (np.random.RandomState(4236).standard_normal((B, 6)) * 2.0 + 1.0).astype(np.float32)
        llr.setflags(write=False)
        return LO.tables(IRREGULAR_NLIST, 5), llr
    if name == 'g768':
        from fgnn_amd.ldpc_code import LdpcCode
        code = LdpcCode.gallager(768, 8, 16, 1)
        return LO.tables(code.nlist, code.n_chk), received(code, 7, (4.0, 4.0), 5)
    code = named_code(name)
    return LO.tables(code.nlist, code.n_chk), received(code, 3000 + CODES.index(name), SNR_DB[name], B)


@functools.lru_cache(maxsize=None)
def restated(name, key, dtype='float32', tol=0.0, tol_r=0.0):
    """The restatement on ``case(name)``'s words with ``SETTINGS[key]``: computed once, shared, never written."""
    tabs, llr = case(name)
    return LP.decode(llr, tabs, dtype=np.dtype(dtype), tol=tol, tol_r=tol_r, **SETTINGS[key])


def soft_error(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max())


# ---- the ML certificate against brute force

def parity_matrix(code):
    H = np.zeros((code.n_chk, code.n_var), np.uint8)
    for n, row in enumerate(code.nlist):
        for m in row:
            if m >= 0:
                H[m, n] ^= 1
    return H


def codewords(H):
    """Every codeword of H [M, N] uint8, [2^k, N] uint8, from a GF(2) null-space basis (Gauss-Jordan elimination)."""
    A, pivots, r = H.copy(), [], 0
    for c in range(A.shape[1]):
        rows = np.nonzero(A[r:, c])[0]
        if not len(rows):
            continue
        A[[r, r + rows[0]]] = A[[r + rows[0], r]]
        for i in np.nonzero(A[:, c])[0]:
            if i != r:
                A[i] ^= A[r]
        pivots.append(c)
        r += 1
        if r == A.shape[0]:
            break
    basis = []
    for c in range(A.shape[1]):
        if c not in pivots:
            v = np.zeros(A.shape[1], np.uint8)
            v[c] = 1
            for i, pc in enumerate(pivots):
                v[pc] = A[i, c]
            basis.append(v)
    basis = np.array(basis, np.int64)
    coef = (np.arange(2 ** len(basis))[:, None] >> np.arange(len(basis))) & 1
    cw = (coef @ basis % 2).astype(np.uint8)
    assert not (cw.astype(np.int64) @ H.T.astype(np.int64) % 2).any()
    return cw


@functools.lru_cache(maxsize=None)
def certificate_case(which, snr):
    """(tables, llr [67, N], the maximum-likelihood codeword of every word [67, N] by enumeration); ``which``: 'g12' (256 codewords)
    or 'g24' = gallager(24, 3, 6, 0) (16384)."""
    from fgnn_amd.ldpc_code import LdpcCode
    code = named_code('g12') if which == 'g12' else LdpcCode.gallager(24, 3, 6, 0)
    cw = codewords(parity_matrix(code))
    assert len(cw) == {'g12': 256, 'g24': 16384}[which]
    llr = received(code, 5000, (snr, snr), B)
    ml = cw[(llr.astype(np.float64) @ cw.T.astype(np.float64)).argmin(1)]
    return LO.tables(code.nlist, code.n_chk), llr, ml


CERTIFICATE_CASES = [('g12', 1.0), ('g12', 3.0), ('g24', 1.0), ('g24', 3.0)]


def assert_certified_words_are_ml(which, snr, x, soft, viol, flags):
    """Every word with flag bit 1 equals argmin_c llr . c over all codewords, has no violated check and soft within 1e-3 of its hard
    decisions; at least 40 words are certified.  Returns their number."""
    _, _, ml = certificate_case(which, snr)
    cert = (np.asarray(flags) & 2) != 0
    assert int(cert.sum()) >= 40, int(cert.sum())
    assert (np.asarray(flags)[cert] & 1).all()
    assert np.array_equal(np.asarray(x)[cert], ml[cert])
    assert not np.asarray(viol)[cert].any()
    assert np.abs(np.asarray(soft, np.float64)[cert] - np.asarray(x)[cert]).max() <= 1e-3
    return int(cert.sum())
