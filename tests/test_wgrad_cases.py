"""CPU: the contract of tests/wgrad_cases.py, which tests/test_wgrad_gpu.py relies on.  fgnn_linear_wgrad_kernel (the query of
include/fgnn_hip_wgrad.h, which chooses through the launch's own code) names, for every case, the kernel the case list says it
reaches -- this pins the dispatch of the weight-gradient families without a device; the expected names are all the variants there are;
the exact data sets are exact (an integer reference below 2^24 that an f32 product reproduces in two row orders); and the piece sets
exercise the pieces they claim to."""
import ctypes
import os
import re

import pytest
import torch

import wgrad_cases as C

IDS = [c['id'] for c in C.CASES]


def query(dtype, shape, xbits=0, gybits=0):
    from fgnn_amd import _hip
    code = _hip.F32 if dtype == C.F32 else _hip.BF16
    return _hip.invoke('fgnn_linear_wgrad_kernel', shape[0], shape[1], shape[2], code, xbits, gybits).decode()


def test_the_query_is_a_bound_companion_of_the_main_header():
    from fgnn_amd import _hip
    NEW = ('fgnn_linear_wgrad_kernel',)
    text = open(os.path.join(os.path.dirname(_hip.HEADER_PATH), 'fgnn_hip_wgrad.h')).read()
    sig = _hip.signatures(text)
    assert tuple(sig) == NEW == _hip.WGRAD
    assert not set(NEW) & set(_hip.EXPORTS) and not set(NEW) & set(_hip.SIGNATURES) and _hip.ABI_VERSION == 15
    main = open(_hip.HEADER_PATH).read()
    assert not any(re.search(r'\b%s\b' % name, main) for name in NEW)
    L = _hip.lib()
    fn = getattr(L, NEW[0])                                          # exported by the built library ...
    restype, params = sig[NEW[0]]
    assert fn.restype is restype is ctypes.c_char_p                  # ... and bound with the parsed types
    assert list(fn.argtypes) == [t for _, t in params] and _hip.COMPANIONS[NEW[0]][:2] == sig[NEW[0]]
    assert params == [('R', ctypes.c_int64), ('Cin', ctypes.c_int32), ('Cout', ctypes.c_int32), ('dtype', ctypes.c_int32),
                      ('x_low_bits', ctypes.c_int32), ('gy_low_bits', ctypes.c_int32)]
    assert text.count('No counterpart in the reference') >= len(NEW)


@pytest.mark.parametrize('cid', IDS)
def test_the_query_names_the_kernel_the_case_reaches(cid):
    c = C.BY_ID[cid]
    esz = 4 if c['dtype'] == C.F32 else 2
    assert query(c['dtype'], c['shape'], c['xoff'] * esz & 15, c['gyoff'] * esz & 15) == c['kernel'], c['reaches']
    if c['xoff'] or c['gyoff']:                                      # the offset is what keeps the aligned shape's kernel away
        assert query(c['dtype'], c['shape']) != c['kernel']


def test_every_kernel_variant_is_some_cases_expectation():
    assert sorted({c['kernel'] for c in C.CASES}) == C.ALL_KERNELS == sorted([
        'linear_wgrad_kernel<float>', 'linear_wgrad_kernel<bf16>',
        'linear_wgrad_vec_kernel<float, 4, 4>', 'linear_wgrad_vec_kernel<float, 16, 10>',
        'linear_wgrad_vec_kernel<bf16, 4, 4>', 'linear_wgrad_vec_kernel<bf16, 16, 10>',
        'linear_wgrad_b16_narrow_kernel<true>', 'linear_wgrad_b16_narrow_kernel<false>',
        'linear_wgrad_b16_kernel S=1', 'linear_wgrad_b16_kernel S=2', 'linear_wgrad_b16_kernel S=4', 'linear_wgrad_b16_kernel S=8',
        'linear_wgrad_b16_kernel S=16', 'linear_wgrad_lds_kernel S=8', 'linear_wgrad_lds_kernel S=16',
        'linear_wgrad_f32q_kernel<64, 64>', 'linear_wgrad_f32q_kernel<64, 128>', 'linear_wgrad_f32q_kernel<128, 64>',
        'linear_wgrad_f32q_kernel<128, 128>'])
    assert any(c['gb_null'] for c in C.CASES if c['family'] == 'f32') and any(c['gb_null'] for c in C.CASES if c['family'] == 'narrow')
    assert {c['family'] for c in C.CASES} == {'general', 'narrow', 'b16', 'f32'}


def test_the_query_refuses_what_no_family_takes_and_keeps_no_state():
    from fgnn_amd import _hip
    L = _hip.lib()
    for dtype, shape in C.REFUSED:
        assert query(dtype, shape) == ''
        assert int(L.fgnn_linear_wgrad_workspace_bytes(*shape)) == -1
    before = L.fgnn_last_kernel()
    assert query(C.F32, (0, 64, 64)) == '' and query(C.F32, (300, 0, 64)) == '' and query(C.F32, (300, 64, -1)) == ''
    assert _hip.invoke('fgnn_linear_wgrad_kernel', 300, 64, 64, 7, 0, 0) == b''              # an unknown storage type
    assert query(C.F32, (2 ** 31, 64, 64)) == ''
    # the pair either side of the f32 family's row threshold, and the same answer however often it is asked
    assert query(C.F32, (2047, 64, 64)) == 'linear_wgrad_vec_kernel<float, 16, 10>'
    assert [query(C.F32, (2048, 64, 64)) for _ in range(3)] == ['linear_wgrad_f32q_kernel<64, 64>'] * 3
    # only the low four bits of an offset count
    assert query(C.BF16, (2085, 128, 256), 8 + 16) == query(C.BF16, (2085, 128, 256), 8) == 'linear_wgrad_b16_kernel S=8'
    assert L.fgnn_last_kernel() == before                           # what whole passes read afterwards is not the query's to write


@pytest.mark.parametrize('cid', IDS)
def test_exact_data_sets_are_exact_and_rand_is_finite(cid):
    c = C.BY_ID[cid]
    R = c['shape'][0]
    assert 9 * R + 2 < C.LIMIT
    for name in C.EXACT_SETS[c['dtype']]:
        x, gy = C.make(c, name)
        assert x.dtype == gy.dtype == C.DTYPE[c['dtype']]
        rw, rb = C.reference(x, gy)
        for ref in (rw, rb):
            assert torch.equal(ref, ref.round()) and float(ref.abs().max()) + max(C.GW0, C.GB0) < C.LIMIT, name
        xf, gf = x.float(), gy.float()
        assert torch.equal((gf.t() @ xf).double(), rw) and torch.equal((gf.flip(0).t() @ xf.flip(0)).double(), rw), name
        assert torch.equal(gf.sum(0).double(), rb) and torch.equal(gf.flip(0).sum(0).double(), rb), name
        if name != 'ints':
            nz = (gy != 0).sum(0)
            assert torch.equal(nz, torch.ones_like(nz)), name        # one non-zero row per column: every gW element is one product
            rows = (gy != 0).double().argmax(0).tolist()
            edges = C.edge_rows(c)[:c['shape'][2]]
            assert rows[:len(edges)] == edges and 0 in rows
    x, gy = C.make(c, 'rand')
    rw, rb = C.reference(x, gy)
    assert bool(torch.isfinite(rw).all()) and bool(torch.isfinite(rb).all()) and float(rw.abs().max()) > 0
    x2, _ = C.make(c, 'rand')
    assert torch.equal(x, x2)                                        # the generators are functions of (case, set)


def test_piece_sets_need_the_pieces_they_name():
    """An odd integer below 2^12 is two bf16 pieces (one only where it is below 2^8: 1 draw in 16) and never three, an odd one below
    2^20 three in 69 % of the draws (round-to-nearest pieces hold 17 to 18 bits between two) with nothing left after the third, a power of two is one: so p12 fails without h.m / m.h / m.m, p20x without
    x's l piece, p20g without gy's."""
    c = C.BY_ID['Q2']
    x12, g12 = C.make(c, 'p12')
    (h, m, l), rest = C.pieces(x12)
    assert float((m != 0).double().mean()) > 0.9 and not bool(l.any()) and not bool(rest.any())
    (h, m, l), rest = C.pieces(g12)
    nz = g12 != 0
    assert float((m[nz] != 0).double().mean()) > 0.8 and not bool(l.any()) and not bool(rest.any())
    assert float(x12.abs().max()) <= 4095 and float(g12.abs().max()) <= 4095
    x20, g20 = C.make(c, 'p20x')
    (h, m, l), rest = C.pieces(x20)
    assert float((l != 0).double().mean()) > 0.6 and not bool(rest.any()) and float(x20.abs().max()) < 2 ** 20
    (h, m, l), rest = C.pieces(g20)
    assert not bool(m.any()) and not bool(l.any()) and set(g20.abs().unique().tolist()) <= {0.0, 1.0, 2.0, 4.0, 8.0}
    x20, g20 = C.make(c, 'p20g')
    (h, m, l), rest = C.pieces(g20)
    nz = g20 != 0
    assert float((l[nz] != 0).double().mean()) > 0.5 and not bool(rest.any())     # (64 draws)
    (h, m, l), rest = C.pieces(x20)
    assert not bool(m.any()) and not bool(l.any())


def test_edge_rows_follow_the_plans_row_split():
    """rows_per_workgroup restates the two f32 plans' row split; the workspace the library asks for pins it where one family alone
    sizes it: gx slabs of (Cout Cin + Cout) floats for the piece form."""
    from fgnn_amd import _hip
    L = _hip.lib()
    for cid in ('Q1', 'Q2', 'Q5'):
        c = C.BY_ID[cid]
        R, cin, cout = c['shape']
        gx = -(-R // C.rows_per_workgroup(c))
        assert int(L.fgnn_linear_wgrad_workspace_bytes(R, cin, cout)) >= gx * (cout * cin + cout) * 4
    assert C.rows_per_workgroup(C.BY_ID['Q5']) == 544 and C.rows_per_workgroup(C.BY_ID['Q1']) == 64
    assert C.rows_per_workgroup(C.BY_ID['G15a']) == 128 and C.rows_per_workgroup(C.BY_ID['G3']) == 64
    assert C.edge_rows(C.BY_ID['G15a']) == [0, 32840, 32768 + 31, 32768 + 32, 32768 + 63, 32768 + 64, 31, 32, 63, 64]
