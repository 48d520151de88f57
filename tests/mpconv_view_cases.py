"""The message operator on strided, offset and batch-shared operand VIEWS: the one dimension tests/mpconv_sg_cases.py and
tests/mpconv_b16_cases.py leave out.  Those vary shapes, degrees and batch sizes; here the shapes stay put and what varies is WHERE an
operand lies in memory -- the thing the layout rules of the twelve plans (six forward, six backward families: csrc/mpconv_fwd*.hip,
csrc/mpconv_bwd*.hip) decide on.  A helper module like the two above, whose references and bounds it reuses; not a test module.
tests/test_mpconv_view_cases.py (CPU) checks the builders, the references and that every layout rule is named;
tests/test_mpconv_views_gpu.py runs the table.

A case is (call kind, batch size, view geometry, mode).  ``KINDS`` has one call kind per family at the smallest shape it still runs at;
``GEOMETRIES`` the places an operand can lie: ONE operand is a view per case and the others are dense, plus three combined ones.  Every
view lies inside one base allocation filled with a fixed NaN bit pattern (``PATTERN``; an index base holds an id far out of range, which
the kernels clamp), with at least ``SLACK`` elements of it on both sides of everything the view covers: a kernel that ignored a stride
would read NaNs, not fault.  ``expect`` names, for the forward and the backward of every case, the kernel ``fgnn_last_kernel`` must
report and -- where the family of the dense control turns the view down -- the rules that do so ("ws forward 11"), as read from the
plans as coded today.  ``RULES`` is the list of layout rules of the twelve plans, written out by hand (not scraped), so that a rule
added later without a case fails the CPU test.

Modes: 'fwd' (ops.mpconv_forward_raw), 'bwd' (ops.mpconv and its backward), 'stats' (the training-mode call whose epilogue leaves the
BatchNorm's statistics: the table-driven shapes and F8 of mpconv_b16_cases).  Backward cases exist only for the geometries the Python
layer lets through to the kernels: ``_MPConv.backward`` copies a non-dense x and copies gz into its own layout, so they are the
offset-but-dense x views and every etype and nn_idx geometry.  For the same reason the backward plans' x-stride rules and every rule
on y, gz, argmax, gx, getype and the workspace cannot be reached from Python: ``OUT_OF_REACH`` lists them; ``OTHER_LAYOUT``
the three forward rules that, taking every view of a channel-fastest operand, are left with the suite's other layout.

f32 kinds: an offset of "2 bytes" is one element (4 bytes).  The hyper-edge kinds take no edge-type gradient (their etype is a
constant in the models, and only then does the hyper-edge backward run)."""
import torch

import mpconv_b16_cases as C
import mpconv_sg_cases as S

SLACK = 64                                     # elements of guard band on each side of a view
B_SMALL, B_LARGE = 5, 300                      # 300: the table-driven grid is 256, so 44 workgroups take a second sample
PATTERN = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5), torch.int64: (torch.int64, 0x7FA5A5A5A5A5A5A5)}
BF16, F32 = torch.bfloat16, torch.float32

# name: (dtype, (nin, nou, net, N, M, k), ext, group, table, nn_idx shared by the batch, etype shared, etype takes a gradient)
KINDS = {
    'ws6':      (BF16, (64, 64, 4, 96, 48, 6), 0, 'ws', 'bounded', True, False, True),
    'ws3k':     (BF16, (128, 64, 4, 48, 96, 3), 0, 'ws', 'bounded', True, False, True),
    'ws6x2':    (BF16, (64, 128, 4, 96, 48, 6), 0, 'ws', 'bounded', True, False, True),       # two launches
    'b16':      (BF16, (64, 64, 4, 96, 48, 6), 0, 'b16', 'relabelled', False, False, True),   # per-sample tables
    'fanin':    (BF16, (64, 64, 1, 96, 1, 96), 0, 'fanin', 'permutation', True, False, False),
    'fanin_id': (BF16, (64, 64, 1, 96, 1, 96), 0, 'fanin', 'identity', True, False, False),
    'fanout':   (BF16, (64, 64, 1, 1, 96, 1), 0, 'fanout', 'zero', True, False, False),
    'ext1':     (F32, (64, 64, 16, 1, 1, 1), 1, 'ext', 'random', True, True, True),           # the smallest of test_mpconv_ext_gpu.SHAPES
    'ext2':     (F32, (64, 64, 16, 1, 1, 1), 2, 'ext', 'random', True, True, True),
    'ext2w':    (F32, (64, 64, 16, 33, 33, 3), 2, 'ext', 'random', True, True, True),         # and one with neighbours to gather
    'res':      (F32, (64, 64, 4, 96, 48, 6), 0, 'res', 'random', False, False, True),        # an f32 LDPC shape
    'generic':  (F32, (12, 10, 4, 20, 13, 3), 0, 'generic', 'random', False, False, True),    # 40 columns: only the generic kernels
    'F8':       (BF16, C.SHAPE['F8'], 0, 'b16', 'random', False, False, True),                # statistics epilogue below 64 channels
}
STATS_KINDS = ('ws6', 'ws3k', 'ws6x2', 'F8')
LARGE_FWD = ('ws6', 'ws3k', 'ws6x2', 'b16')    # forward and statistics also at B_LARGE
LARGE_BWD = ('ws6', 'b16')                     # backward also at B_LARGE

# geometry: operand -> how its view differs from dense.  off: bytes past a 16-byte boundary; sb_pad: elements added to the sample
# stride; every: a [::2] of a base; sn_pad: channels added to a row; row_pad: neighbour slots added to a destination's edge-type row;
# col_pad: columns added to the table; row_off: rows in front of the table; expand: batch stride 0; copies: B equal copies
GEOMETRIES = {
    'dense': {},
    'x+1el': {'x': {'off_el': 1}}, 'x+8B': {'x': {'off': 8}}, 'x_sb+8': {'x': {'sb_pad': 8}}, 'x_sb+4': {'x': {'sb_pad': 4}},
    'x[::2]': {'x': {'every': 2}}, 'x_chslice': {'x': {'sn_pad': 16}}, 'x_expand': {'x': {'expand': True}},
    'et+8B': {'et': {'off': 8}}, 'et+2B': {'et': {'off': 2}}, 'et_sb+2': {'et': {'sb_pad': 2}}, 'et_sb+4': {'et': {'sb_pad': 4}},
    'et_sb+8': {'et': {'sb_pad': 8}},
    'et_expand': {'et': {'expand': True}}, 'et_rowpad': {'et': {'row_pad': 1}},
    'idx_colslice': {'idx': {'col_pad': 1}}, 'idx_rowoff': {'idx': {'row_off': 1}}, 'idx_expand': {'idx': {'expand': True}},
    'idx_copies': {'idx': {'copies': True}},
    'x+1el&et+2B': {'x': {'off_el': 1}, 'et': {'off': 2}}, 'x+8B&et+8B': {'x': {'off': 8}, 'et': {'off': 8}},
    'x_sb+8&et_sb+4': {'x': {'sb_pad': 8}, 'et': {'sb_pad': 4}},
}
# the geometries whose x the backward is handed as it is (dense, possibly offset); the others' x is copied by _MPConv.backward
BWD_X = ('dense', 'x+1el', 'x+8B')

# The layout rules of the twelve plans: every rule that mentions a stride or a pointer, by the name FGNN_TRACE prints ("family
# rule") or, for the unnumbered ``return 0`` lines, "family operand".  Written out by hand, as coded today.
RULES = [
    'hyper-edge forward 4', 'hyper-edge forward 5',
    'ws forward 6', 'ws forward 7', 'ws forward 8', 'ws forward 9', 'ws forward 10', 'ws forward 11',
    'b16 forward x', 'b16 forward y', 'b16 forward et',
    'ext forward x', 'ext forward y', 'ext forward shared',
    'res forward x', 'res forward et',
    'ext backward shared', 'ext backward x', 'ext backward y', 'ext backward pointers',
    'hyper-edge backward 5', 'hyper-edge backward packed',
    'ws backward 6', 'ws backward 7', 'ws backward 8', 'ws backward 9', 'ws backward 10', 'ws backward 13',
    'bf16-MFMA backward 4', 'bf16-MFMA backward 5', 'bf16-MFMA backward 6', 'bf16-MFMA backward 8',
    'resident backward 8', 'resident backward 9', 'resident backward 10', 'resident backward 11', 'resident backward 15/16/99',
]
# rules no case reaches.  No Python caller can: ops allocates y, argmax, gx, getype and the workspace itself and copies gz into y's layout, and
# _MPConv.backward copies a non-dense x (a dense x of 64 or 128 channels has a sample stride that is a multiple of 8)
OUT_OF_REACH = {
    'hyper-edge forward 5': 'y', 'ws forward 9': 'y', 'b16 forward y': 'y', 'ext forward y': 'y',
    'ext backward y': 'gz', 'hyper-edge backward 5': 'gz', 'ws backward 9': 'gz', 'bf16-MFMA backward 5': 'gz',
    'resident backward 10': 'gz', 'resident backward 11': 'gz',
    'ext backward x': 'x is dense in the backward', 'ws backward 8': 'x is dense in the backward',
    'bf16-MFMA backward 4': 'x is dense in the backward', 'resident backward 8': 'x is dense in the backward',
    'resident backward 9': 'x is dense in the backward',
}
# rules a view of a channel-fastest x / edge-type-fastest etype cannot reach since these plans take any row stride, sample stride and
# address of one: they turn down the suite's other layout (node-fastest x, which the resident kernels take with f32 projections) or
# no layout at all.  Where that layout is run: tests/test_mpconv_gpu.py::test_layouts_and_shared_graph_vs_oracle and
# tests/test_fanin_bwd_gpu.py::test_layouts_without_16_byte_rows (nchw), tests/test_mpconv_b16_gpu.py (plain etype, which
# mpconv_fwd_b16 takes).
OTHER_LAYOUT = {
    'hyper-edge forward 4': 'node-fastest x', 'b16 forward x': 'node-fastest x',
    'b16 forward et': 'neither edge-type fastest nor plain',
}

_FWD_GEN, _BWD_GEN = 'mpconv_fwd_kernel<%s, %d, 0>', 'mpconv_bwd_kernel<%s, %d, 0>'


def _names(kind):
    """family -> kernel name of a kind, forward and backward, as the launch functions print them."""
    dtype, shape, ext, group = KINDS[kind][:4]
    nin, nou, net, N, M, k = shape
    t = 'bf16_t' if dtype == BF16 else 'float'
    fwd, bwd = {'gen': _FWD_GEN % (t, net)}, {'gen': _BWD_GEN % (t, net)}
    ncols = nou * net
    if net in (1, 4) and ext == 0 and ncols % 16 == 0:
        swp, npass = ((ncols if ncols <= 256 else 256) // 16 + 7) // 8, (ncols + 255) // 256
        fwd['res'] = 'mpconv_fwd_res_kernel<%s, %d, 0, %d, %d, %d>' % (t, net, (nin + 63) // 64 * 16, swp, npass)
        bnp = (ncols + 127) // 128
        bwd['res'] = 'mpconv_bwd_res_kernel<%s, %d, %d, %d, %s>' % (t, net, nin // 4, bnp, 'true' if nin == 64 and bnp <= 2 else 'false')
    if dtype == BF16 and C.plan_model(shape) is not None:
        fwd['b16'] = C.forward_kernel(shape, 'max')
        bwd['b16'] = 'mpconv_bwd_b16_kernel<%d, %d>' % (nin // 32, nou // 32)
    if group == 'ws':
        sfx = ' x2' if nou == 128 else ''
        fwd['ws'] = 'mpconv_fwd_ws_kernel<%d, %d, 0, %d>%s' % (nin, k, 3 if nin == 64 else 2, sfx)
        fwd['ws+stats'] = 'mpconv_fwd_ws_kernel<%d, %d, 1, %d>%s' % (nin, k, 3 if nin == 64 else 2, sfx)
        bwd['ws'] = 'mpconv_bwd_ws_kernel<%d, %d>%s' % (k, 3 if k == 6 else 6, sfx or (' k2' if nin == 128 else ''))
    if kind == 'b16':                           # a batch-shared table sends the per-sample kind to the table-driven family
        fwd['ws'], bwd['ws'] = _names('ws6')[0]['ws'], _names('ws6')[1]['ws']
    if group == 'fanin':
        fwd['hyper'] = 'mpconv_fwd_fanin_id_kernel<2, 4>' if kind == 'fanin_id' else 'mpconv_fwd_fanin_kernel<0, 2, 4>'
        bwd['hyper'] = 'mpconv_bwd_fanin_kernel<bf16_t, 1, 1>'
    if group == 'fanout':
        fwd['hyper'], bwd['hyper'] = 'mpconv_fwd_fanout_kernel<1, 4>', 'mpconv_bwd_fanout_kernel<bf16_t, 1, 1>'
    if group == 'ext':
        fwd['ext'], fwd['extn'] = 'mpconv_fwd_extp_kernel<0, false>', 'mpconv_fwd_ext_kernel<0>'
        bwd['ext'] = 'mpconv_bwd_extq_kernel<2, '          # (prefix: the separate dP image is an LDS question)
    return fwd, bwd


_WS11, _WSB13 = ('ws forward 11',), ('ws backward 13', 'bf16-MFMA backward 8')
_ET_B = ('bf16-MFMA backward 6', 'resident backward 15/16/99')
# group -> geometry -> (forward family, the rules that turned the control's family down, backward family or None, its rules)
GROUPS = {
    'ws': {
        'dense': ('ws', (), 'ws', ()),
        'x+1el': ('b16', _WS11, 'res', _WSB13), 'x+8B': ('b16', _WS11, 'res', _WSB13),
        'x_sb+8': ('ws', (), None, ()), 'x_sb+4': ('b16', ('ws forward 8',), None, ()),
        'x[::2]': ('ws', (), None, ()), 'x_chslice': ('b16', ('ws forward 8',), None, ()),
        'x_expand': ('ws', (), None, ()),
        'et+8B': ('b16', _WS11, 'ws', ()),          # the backward reads an edge's four types as one 8-byte word: rule 13 wants 8 bytes
        'et+2B': ('b16', _WS11, 'res', _WSB13),
        'et_sb+2': ('b16', ('ws forward 10',), 'res', ('ws backward 10', 'bf16-MFMA backward 6')),   # no 8-byte words: the % 4 of both rules
        'et_sb+4': ('b16', ('ws forward 10',), 'ws', ()),       # and its rule 10 a sample stride of 4 elements = those 8 bytes
        'et_sb+8': ('ws', (), 'ws', ()), 'et_expand': ('ws', (), 'ws', ()),
        'et_rowpad': ('b16', ('ws forward 10',), 'gen', ('ws backward 10',) + _ET_B),
        'idx_colslice': ('b16', ('ws forward 7',), 'b16', ('ws backward 7',)),
        'idx_rowoff': ('ws', (), 'ws', ()), 'idx_copies': ('ws', (), 'ws', ()),
        'x+1el&et+2B': ('b16', _WS11, 'res', _WSB13), 'x+8B&et+8B': ('b16', _WS11, 'res', _WSB13),
        'x_sb+8&et_sb+4': ('b16', ('ws forward 10',), None, ()),
    },
    'b16': {
        'dense': ('b16', ('ws forward 6',), 'b16', ('ws backward 6',)),
        'x+1el': ('b16', (), 'res', ('bf16-MFMA backward 8',)), 'x+8B': ('b16', (), 'res', ('bf16-MFMA backward 8',)),
        'x_sb+8': ('b16', (), None, ()), 'x_sb+4': ('b16', (), None, ()), 'x[::2]': ('b16', (), None, ()),
        'x_chslice': ('b16', (), None, ()), 'x_expand': ('b16', (), None, ()),
        'et+8B': ('b16', (), 'b16', ()), 'et+2B': ('b16', (), 'res', ('bf16-MFMA backward 8',)),
        'et_sb+2': ('b16', (), 'res', ('bf16-MFMA backward 6',)),
        'et_sb+4': ('b16', (), 'b16', ()), 'et_sb+8': ('b16', (), 'b16', ()), 'et_expand': ('b16', (), 'b16', ()),
        'et_rowpad': ('b16', (), 'gen', _ET_B),
        'idx_colslice': ('b16', (), 'b16', ()), 'idx_rowoff': ('b16', (), 'b16', ()), 'idx_expand': ('ws', (), 'ws', ()),
        'x+1el&et+2B': ('b16', (), 'res', ('bf16-MFMA backward 8',)), 'x+8B&et+8B': ('b16', (), 'res', ('bf16-MFMA backward 8',)),
        'x_sb+8&et_sb+4': ('b16', (), None, ()),
    },
    'fanin': {
        'dense': ('hyper', (), 'hyper', ()),
        'x+1el': ('hyper', (), 'hyper', ('hyper-edge backward packed',)),          # (the backward: element accesses, same kernel)
        'x+8B': ('hyper', (), 'hyper', ('hyper-edge backward packed',)),
        'x_sb+8': ('hyper', (), None, ()), 'x_sb+4': ('hyper', (), None, ()),
        'x[::2]': ('hyper', (), None, ()), 'x_chslice': ('hyper', (), None, ()),
        'x_expand': ('hyper', (), None, ()),
        'et+8B': ('hyper', (), 'hyper', ()), 'et+2B': ('hyper', (), 'hyper', ()), 'et_sb+2': ('hyper', (), 'hyper', ()),
        'et_sb+4': ('hyper', (), 'hyper', ()),
        'et_sb+8': ('hyper', (), 'hyper', ()), 'et_expand': ('hyper', (), 'hyper', ()),
        'idx_colslice': ('hyper', (), 'hyper', ()), 'idx_rowoff': ('hyper', (), 'hyper', ()), 'idx_copies': ('hyper', (), 'hyper', ()),
        'x+1el&et+2B': ('hyper', (), 'hyper', ('hyper-edge backward packed',)),
        'x+8B&et+8B': ('hyper', (), 'hyper', ('hyper-edge backward packed',)),
        'x_sb+8&et_sb+4': ('hyper', (), None, ()),
    },
    'ext': {
        'dense': ('ext', (), 'ext', ()),
        'x+1el': ('gen', ('ext forward x',), 'gen', ('ext backward pointers',)),
        'x+8B': ('gen', ('ext forward x',), 'gen', ('ext backward pointers',)),
        'x_sb+8': ('ext', (), None, ()), 'x_sb+4': ('ext', (), None, ()), 'x[::2]': ('ext', (), None, ()),
        'x_chslice': ('gen', ('ext forward x',), None, ()), 'x_expand': ('ext', (), None, ()),
        'et+8B': ('ext', (), 'ext', ()), 'et+2B': ('ext', (), 'ext', ()),
        'et_sb+2': ('extn', ('ext forward shared',), 'gen', ('ext backward shared',)),
        'et_sb+4': ('extn', ('ext forward shared',), 'gen', ('ext backward shared',)),        # per-sample edge types
        'et_sb+8': ('extn', ('ext forward shared',), 'gen', ('ext backward shared',)),
        'idx_colslice': ('ext', (), 'ext', ()), 'idx_rowoff': ('ext', (), 'ext', ()), 'idx_copies': ('ext', (), 'ext', ()),
        'x+1el&et+2B': ('gen', ('ext forward x',), 'gen', ('ext backward pointers',)),
        'x+8B&et+8B': ('gen', ('ext forward x',), 'gen', ('ext backward pointers',)),
        'x_sb+8&et_sb+4': ('extn', ('ext forward shared',), None, ()),
    },
}
# one source node (fan-out), the resident f32 kernels and the generic ones read every operand by element strides: no view moves them
_X = ('x+1el', 'x+8B', 'x_sb+8', 'x_sb+4', 'x[::2]', 'x_chslice', 'x_expand')
_ET = ('et+8B', 'et+2B', 'et_sb+2', 'et_sb+4', 'et_sb+8', 'et_expand', 'et_rowpad')
_COMBINED = ('x+1el&et+2B', 'x+8B&et+8B', 'x_sb+8&et_sb+4')


def _flat(family, idx_geoms, moved=None):
    g = {n: (family, (), family if (n in BWD_X or n[0] in 'ei' or n in _COMBINED[:2]) else None, ()) for n in
         ('dense',) + _X + _ET + idx_geoms + _COMBINED}
    g.update(moved or {})
    return g


GROUPS['fanout'] = _flat('hyper', ('idx_colslice', 'idx_rowoff', 'idx_copies'))
GROUPS['res'] = _flat('res', ('idx_colslice', 'idx_rowoff', 'idx_expand'), {
    'x_chslice': ('gen', ('res forward x',), None, ()), 'et_rowpad': ('gen', ('res forward et',), 'gen', ('resident backward 15/16/99',))})
GROUPS['generic'] = _flat('gen', ('idx_colslice', 'idx_rowoff', 'idx_expand'))


def expect(kind, geometry):
    """dict(fwd, fwd_rules, bwd (None: no backward case), bwd_rules) of one case: kernel names and the rules that moved it."""
    ff, fr, bf, br = GROUPS[KINDS[kind][3]][geometry]
    fwd, bwd = _names(kind)
    if ff == 'ws' and 'ws' not in fwd:          # F8 with a batch-shared table: k = 5 is no table-driven shape ("ws forward 2")
        ff, bf = 'b16', 'b16'
    return dict(fwd=fwd[ff], fwd_rules=fr, bwd=None if bf is None else bwd[bf], bwd_rules=br, fwd_family=ff, bwd_family=bf)


def expect_stats(kind, geometry):
    """(kernel of the training-mode forward, True when its epilogue leaves the statistics / False when a bn_stats pass follows the
    plain forward).  ops.mpconv_forward_raw asks for the epilogue only with 16-byte aligned x and etype (the table-driven plan's
    rule 11 cannot hand a statistics call on: the partial rows were announced for its grid); the pointer-free plan
    (fgnn_mpconv_forward_stats_partials) decides the rest: the table-driven kernel, mpconv_fwd_b16 at up to 64 channels, or none."""
    e = expect(kind, geometry)
    nou = KINDS[kind][1][1]
    spec = GEOMETRIES[geometry]
    if any(('off' in spec.get(o, {}) or 'off_el' in spec.get(o, {})) for o in ('x', 'et')):
        return e['fwd'], False
    if e['fwd_family'] == 'ws':
        return _names(kind)[0]['ws+stats'], True
    if e['fwd_family'] == 'b16' and nou <= 64:
        return e['fwd'], True
    return e['fwd'], False


def cases():
    """[(kind, B, geometry, mode)]: the table (a kind's runs at one batch size stand together: they share their references)."""
    out = []
    for kind in KINDS:
        group = KINDS[kind][3]
        for B in (B_SMALL, B_LARGE):
            for geometry in GROUPS[group]:
                e = expect(kind, geometry)
                if kind != 'F8':
                    if B == B_SMALL or kind in LARGE_FWD:
                        out.append((kind, B, geometry, 'fwd'))
                    if e['bwd'] is not None and (B == B_SMALL or kind in LARGE_BWD):
                        out.append((kind, B, geometry, 'bwd'))
                if kind in STATS_KINDS and (B == B_SMALL or kind in LARGE_FWD):
                    out.append((kind, B, geometry, 'stats'))
    return out


def case_id(c):
    return '%s-B%d-%s-%s' % c


# Per-node / per-edge yardstick of the bf16 backward cases with an edge-type gradient, as tests/mpconv_sg_cases.py defines D_NODE /
# D_EDGE and tests/mpconv_b16_cases.py its D: the routed reference with the kernels' rounding points against the unrounded one, at
# B = 5 -- measured on the CPU by tests/test_mpconv_view_cases.py::test_rounding_model_error, which asserts these values hold.
# (d_node, d_edge), the measurement rounded up by about 1 %:
D = {
    'ws6':   (4.53e-03, 6.51e-03),      # measured 4.4784e-03, 6.4376e-03
    'ws3k':  (4.31e-03, 5.18e-03),      # measured 4.2623e-03, 5.1225e-03
    'ws6x2': (4.51e-03, 6.19e-03),      # measured 4.4628e-03, 6.1201e-03
    'b16':   (4.39e-03, 6.00e-03),      # measured 4.3419e-03, 5.9313e-03
}
HYPER_TOL = 2.0 ** -7                          # tests/test_fanin_bwd_gpu.py: dx, dW, dbias of the hyper-edge backward (bf16)
F32_TOL = {'ext': 2e-4}                        # tests/test_mpconv_ext_gpu.py's backward bound; the other f32 kinds: 1e-4
STATS_TOL = dict(y=2.0 ** -7, mean=1e-5, var=1e-4)      # test_bf16_forward_statistics_epilogue_feeds_batchnorm


# ----------------------------------------------------------------------------------------------------------------------------------
# values
# ----------------------------------------------------------------------------------------------------------------------------------
def problem(kind, B, seed=0):
    """The values of one kind as CPU tensors in the natural layouts (x [B, N, nin], idx [1 or B, M, k], et [1 or B, M, k, net],
    gz [B, M, nou]; bf16 kinds: bf16 values, W holds bf16 values in f32): a dict."""
    dtype, shape, ext, group, table, sh_idx, sh_et, _ = KINDS[kind]
    nin, nou, net, N, M, k = shape
    g = torch.Generator().manual_seed(seed + 3000 + N + 7 * M + 13 * nou + 17 * k + nin + net + B + 101 * ext)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype)
    x = rnd(B, N, nin)
    if table == 'bounded':
        idx, _ = S.bounded_table(N, M, k, S.DEG[k], g, S.empties_for(N, M, k))
    elif table == 'relabelled':                 # per-sample tables with the in-degree profile of one bounded table
        base, _ = S.bounded_table(N, M, k, S.DEG[k], g, S.empties_for(N, M, k))
        idx = torch.stack([torch.randperm(N, generator=g)[base[0]] for _ in range(B)])
        idx[0] = base[0]
    elif table == 'permutation':
        idx = torch.randperm(N, generator=g).reshape(1, 1, N)
    elif table == 'identity':
        idx = torch.arange(N).reshape(1, 1, N)
    elif table == 'zero':
        idx = torch.zeros(1, M, k, dtype=torch.int64)
    else:
        idx = torch.randint(0, N, (1 if sh_idx else B, M, k), generator=g)
    et = rnd(1 if sh_et else B, M, k, net)
    R = nin if ext == 0 else 2 * nin
    W = torch.randn(R, nou * net, generator=g) * 0.1
    if dtype == BF16:
        W = W.bfloat16().float()
    return dict(kind=kind, B=B, x=x, idx=idx, et=et, W=W, bias=torch.randn(nou, generator=g), gz=rnd(B, M, nou))


def values_for(q, geometry):
    """The problem with the rows a batch-expanded operand shares: its first sample's."""
    spec, q = GEOMETRIES[geometry], dict(q)
    for name in ('x', 'et', 'idx'):
        if spec.get(name, {}).get('expand'):
            q[name] = q[name][:1]
    return q


# ----------------------------------------------------------------------------------------------------------------------------------
# builders
# ----------------------------------------------------------------------------------------------------------------------------------
def _base(n, dtype, device):
    t = torch.empty(n, dtype=dtype, device=device)
    as_int, bits = PATTERN[dtype]
    t.view(as_int).fill_(bits)
    assert t.data_ptr() % 16 == 0
    return t


def _strided(values, stride, off_el, device):
    """values as a view of the given element strides, ``off_el`` elements past a 16-byte boundary, inside a fresh base with SLACK
    elements of the pattern on both sides: (view, base)."""
    size = tuple(values.shape)
    extent = 1 + sum((n - 1) * s for n, s in zip(size, stride))
    start = SLACK + off_el
    base = _base(start + extent + SLACK, values.dtype, device)
    view = base.as_strided(size, stride, start)
    view.copy_(values.to(device))
    return view, base


def _off(spec, dtype):
    item = torch.empty(0, dtype=dtype).element_size()
    return spec.get('off_el', 0) + (max(1, spec['off'] // item) if 'off' in spec else 0)


class Operands:
    """x [B, nin, N, 1], idx [B, M, k], et [B, net, M, k] of one call; ``et_leaf``: et before its batch expand ([1 or B, net, M, k]);
    ``bases``: {operand: its base allocation} (empty for the dense clone)."""

    def __init__(self, B, x, idx, et_leaf, bases):
        self.B, self.x, self.idx, self.et_leaf, self.bases = B, x, idx, et_leaf, bases
        self.et = et_leaf.expand(B, -1, -1, -1)


def operands(q, geometry, device):
    """The case's operands as views: the operand(s) the geometry names laid out as it says, the others dense -- every one inside a
    guard-banded base.  ``q``: ``values_for(problem(...), geometry)``."""
    spec, B = GEOMETRIES[geometry], q['B']
    bases = {}
    # x: rows of nin (+ sn_pad) channels, samples N rows (+ sb_pad elements) apart, or every second sample of a base
    sx = spec.get('x', {})
    xv = q['x']
    _, N, nin = xv.shape
    sn = nin + sx.get('sn_pad', 0)
    sb = (N * sn + sx.get('sb_pad', 0)) * sx.get('every', 1)
    x, bases['x'] = _strided(xv, (sb, sn, 1), _off(sx, xv.dtype), device)
    x = x[:, :, None, :].permute(0, 3, 1, 2).expand(B, -1, -1, -1)
    # etype: edge-type fastest, a destination's row k (+ row_pad) slots, samples M rows (+ sb_pad elements) apart
    se = spec.get('et', {})
    ev = q['et']
    if 'sb_pad' in se:                          # (a kind with batch-shared edge types: the same rows once per sample)
        ev = ev.expand(B, -1, -1, -1)
    _, M, k, net = ev.shape
    sm = (k + se.get('row_pad', 0)) * net
    et, bases['et'] = _strided(ev, (M * sm + se.get('sb_pad', 0), sm, net, 1), _off(se, ev.dtype), device)
    et = et.permute(0, 3, 1, 2)
    # nn_idx: rows of k (+ col_pad) columns, row_off rows into a table with that many rows more in front and behind
    si = spec.get('idx', {})
    iv = q['idx'].repeat(B, 1, 1) if si.get('copies') else q['idx']
    ck, ro = k + si.get('col_pad', 0), si.get('row_off', 0)
    idx, bases['idx'] = _strided(iv, ((M + 2 * ro) * ck, ck, 1), ro * ck, device)
    return Operands(B, x, idx.expand(B, -1, -1), et, bases)


def dense_clone(q, device):
    """The same values in fresh, dense, 16-byte aligned tensors of the kind's own form: a batch-shared table / edge types stay shared,
    a batch-expanded operand of a per-sample kind is written out B times."""
    _, _, _, _, _, sh_idx, sh_et, _ = KINDS[q['kind']]
    B = q['B']
    full = lambda t, shared: (t[:1] if shared else t.expand(B, *t.shape[1:])).contiguous().to(device)
    x = full(q['x'], False)[:, :, None, :].permute(0, 3, 1, 2)
    et = full(q['et'], sh_et).permute(0, 3, 1, 2)
    idx = full(q['idx'], sh_idx).expand(B, -1, -1)
    for t in (x, et, idx):
        assert t.data_ptr() % 16 == 0
    return Operands(B, x, idx, et, {})


def snapshot(o):
    return {n: b.clone() for n, b in o.bases.items()}


def unchanged(o, snap):
    """Every byte of every base is what it was: the guard bands and, the inputs being read-only, the views' insides."""
    return all(torch.equal(b.view(PATTERN[b.dtype][0]), snap[n].view(PATTERN[b.dtype][0])) for n, b in o.bases.items())


def guard_band(view, base):
    """Elements of the base in front of and behind everything the view covers."""
    item = view.element_size()
    first = (view.data_ptr() - base.data_ptr()) // item
    last = first + sum((n - 1) * s for n, s in zip(view.shape, view.stride()))
    return first, base.numel() - 1 - last


# ----------------------------------------------------------------------------------------------------------------------------------
# references (CPU, on operands in the operator's layouts, any strides)
# ----------------------------------------------------------------------------------------------------------------------------------
def _natural(o):
    return o.x[:, :, :, 0].permute(0, 2, 1), o.idx, o.et.permute(0, 2, 3, 1)


def forward_reference(q, o):
    """f64: dict(z [B, M, nou], bound [B, M, nou] the per-element bound, E [B, M, k, nou] the messages).  bf16 kinds:
    mpconv_b16_cases.forward_reference and its derived bound; f32 kinds: the oracle's expression in f64 and 1e-4 of the output range."""
    dtype, shape, ext = KINDS[q['kind']][:3]
    nin, nou, net, N, M, k = shape
    x, idx, et = _natural(o)
    if dtype == BF16:
        r = C.forward_reference(dict(shape=shape, B=o.B, x=x, idx=idx, et=et, W=q['W'], bias=q['bias']), 'max')
        return dict(z=r['z'], bound=r['bound'], E=r['E'])
    import fgnn_oracle as O
    E = O.mp_conv({'filters': q['W'].double()}, '', o.x.double(), o.idx.contiguous(), o.et.double(), nou=nou, net=net, extension=ext,
                  aggregator=None, relu=False).permute(0, 2, 3, 1)
    z = E.amax(2) + q['bias'].double()
    return dict(z=z, bound=torch.full_like(z, 1e-4 * float(z.abs().max())), E=E)


def tie_gap(am, ref, dtype):
    """The near-tie rule of tests/test_mpconv_sg_gpu.py: how far below the maximum the named neighbour's message lies, over the slack
    (2^-6 of the messages' range in bf16, 1e-4 in f32)."""
    E = ref['E']
    gap = float((E.amax(2) - E.gather(2, am.long()[:, :, None, :])[:, :, 0, :]).max())
    return gap / ((2.0 ** -6 if dtype == BF16 else 1e-4) * float(E.abs().max()))


def backward_reference(q, o, am):
    """Autograd through the routing ``am`` [B, M, nou]: (z, gx [B, N, nin], getype [B, M, k, net] per sample, gW, gbias); f32 on the
    bf16 kinds' values (mpconv_sg_cases.routed_reference), f64 through the oracle's expression on the f32 kinds'."""
    dtype, shape, ext = KINDS[q['kind']][:3]
    nin, nou, net, N, M, k = shape
    x, idx, et = _natural(o)
    if dtype == BF16:
        return S.routed_reference(x, idx, et, q['W'], q['bias'], q['gz'], am)
    import fgnn_oracle as O
    xo = o.x.double().contiguous().requires_grad_(True)
    eo = o.et.double().contiguous().requires_grad_(True)
    Wo, bo = q['W'].double().requires_grad_(True), q['bias'].double().requires_grad_(True)
    E = O.mp_conv({'filters': Wo}, '', xo, o.idx.contiguous(), eo, nou=nou, net=net, extension=ext, aggregator=None, relu=False)
    z = E.permute(0, 2, 3, 1).gather(2, am.long()[:, :, None, :])[:, :, 0, :] + bo
    z.backward(q['gz'].double())
    return z.detach(), xo.grad[:, :, :, 0].permute(0, 2, 1), eo.grad.permute(0, 2, 3, 1), Wo.grad, bo.grad


# ----------------------------------------------------------------------------------------------------------------------------------
# the device side
# ----------------------------------------------------------------------------------------------------------------------------------
def _nat_out(t):
    return t.detach().cpu()[:, :, :, 0].permute(0, 2, 1)


def device_forward(q, o):
    """One forward launch on the operands: (z [B, M, nou] as stored (held in f32 / f64), argmax [B, M, nou], kernel name), on the CPU."""
    from fgnn_amd import _hip, ops
    _, shape, ext = KINDS[q['kind']][:3]
    dev = o.x.device
    y, am = ops.mpconv_forward_raw(o.x, o.idx, o.et, q['W'].to(dev), q['bias'].to(dev), shape[1], shape[2], ext, _hip.AGG_MAX, want_argmax=True)
    kern = _hip.lib().fgnn_last_kernel().decode()
    assert y.stride(1) == 1
    return _nat_out(y.float()), _nat_out(am).long(), kern


def device_backward(q, o):
    """Forward and backward through ops.mpconv: (z, argmax, gx, getype or None, gW, gbias, the forward's kernel, the backward's), on the
    CPU in the natural layouts; getype has the batch size of ``o.et_leaf`` (1: summed over the batch)."""
    from fgnn_amd import _hip, ops
    _, shape, ext, _, _, _, _, et_grad = KINDS[q['kind']]
    nou, net = shape[1], shape[2]
    dev = o.x.device
    W, bias = q['W'].to(dev), q['bias'].to(dev)
    _, am = ops.mpconv_forward_raw(o.x, o.idx, o.et, W, bias, nou, net, ext, _hip.AGG_MAX, want_argmax=True)
    xd = o.x.detach().requires_grad_(True)
    ed = o.et_leaf.detach().requires_grad_(et_grad)
    Wd, bd = W.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    z = ops.mpconv(xd, o.idx, ed, Wd, bd, nou, net, ext, _hip.AGG_MAX)
    fwd = _hip.lib().fgnn_last_kernel().decode()
    z.backward(q['gz'].to(dev)[:, :, None, :].permute(0, 3, 1, 2))
    bwd = _hip.lib().fgnn_last_kernel().decode()
    get = ed.grad.float().cpu().permute(0, 2, 3, 1) if et_grad else None
    return _nat_out(z.float()), _nat_out(am).long(), _nat_out(xd.grad.float()), get, Wd.grad.cpu(), bd.grad.cpu(), fwd, bwd
