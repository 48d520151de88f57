"""The weight-gradient kernels of the node-wise maps (csrc/linear_wgrad.hip, linear_wgrad_b16.hip, linear_wgrad_f32.hip) through
fgnn_linear_wgrad: the case list, the data generators, the float64 reference and the bounds that tests/test_wgrad_cases.py (CPU) and
tests/test_wgrad_gpu.py (GPU) share.  A helper module like tests/mpconv_b16_cases.py; not a test module.

A case names the kernel it is meant to reach (``fgnn_linear_wgrad_kernel``, include/fgnn_hip_wgrad.h, must answer with that name: the
CPU test pins the dispatch, the GPU test asks again with the real pointers) and runs with every data set its storage type admits:

``ints``  x and gy dense integers in [-3, 3]: exact in bf16, in f32 and in the first bf16 piece of the f32 piece form.  Every partial
          sum, in any order, is an integer of magnitude <= 9 R + 2 < 2^24 (R <= 270 000, the 2 for the values gW / gb start from), so
          the kernel must return the float64 reference EXACTLY whatever its tiling, slicing and fold order: any indexing, tail,
          masking, slice or fold error shows as a non-zero difference.
``rand``  randn (rounded to bf16 for the bf16 cases) against the bounds tests/test_mpconv_gpu.py has for these entry points: 2e-5 of
          the reference's largest magnitude for f32, that + 1e-5 for bf16, for gW and for gb alike, and bit-identical on a second run.
f32 only, three piece sets.  gy has ONE non-zero row per column, so each gW element is a single product, below 2^24 in magnitude, and
exactness is required again.  The f32 piece form (linear_wgrad_f32q_kernel) cuts both operands into three bf16 pieces h + m + l and
keeps six of the nine piece products; the sets say which of them a correct answer needs:
``p12``   x dense odd 12-bit integers with random signs, gy's non-zeros odd 12-bit integers: both operands split into two pieces (h, m;
          15 draws in 16 -- below 2^8 one piece holds the value) and never three, so the products need h.h, h.m, m.h and m.m.
          |product| <= 4095^2 = 2^24 - 8191.
``p20x``  x dense odd 20-bit integers (the third piece is non-zero for 69 % of them), gy's non-zeros +-2^k, k in 0..3: needs x's l piece.
``p20g``  the roles swapped: gy's non-zeros odd 20-bit integers, x dense +-2^k.
The non-zero rows sit on row 0, row R - 1 and rows 31, 32, 63, 64 of the first and of the last workgroup's row range (the edges of the
kernels' 32- and 64-row tiles), the rest at random rows.

The memory contract (GPU test): every operand is a slice of a larger buffer with 4 KB either side, NaN around x and gy, a fixed bit
pattern (a NaN as f32) around and INSIDE the workspace and around gW / gb; the pointer offsets of the misaligned cases come from the
same slicing."""
import zlib

import torch

F32, BF16 = 'f32', 'bf16'
DTYPE = {F32: torch.float32, BF16: torch.bfloat16}

SCALAR = 'linear_wgrad_kernel<%s>'
VEC_S = 'linear_wgrad_vec_kernel<%s, 4, 4>'
VEC_L = 'linear_wgrad_vec_kernel<%s, 16, 10>'
NARROW_X, NARROW_G = 'linear_wgrad_b16_narrow_kernel<true>', 'linear_wgrad_b16_narrow_kernel<false>'
DIRECT, STAGED = 'linear_wgrad_b16_kernel S=%d', 'linear_wgrad_lds_kernel S=%d'
PIECE = 'linear_wgrad_f32q_kernel<%d, %d>'

# every name the three sources' choosers can return
ALL_KERNELS = sorted([k % t for k in (SCALAR, VEC_S, VEC_L) for t in ('float', 'bf16')] + [NARROW_X, NARROW_G] +
                     [DIRECT % s for s in (1, 2, 4, 8, 16)] + [STAGED % s for s in (8, 16)] +
                     [PIECE % bb for bb in ((64, 64), (64, 128), (128, 64), (128, 128))])


def _t(dtype):
    return 'float' if dtype == F32 else 'bf16'


CASES = []      # dicts: id, dtype, shape (R, Cin, Cout), xoff / gyoff (elements), gb_null, kernel, family, reaches


def _case(cid, dtype, shape, kernel, reaches, xoff=0, gyoff=0, gb_null=False):
    family = ('general' if kernel.startswith(('linear_wgrad_kernel', 'linear_wgrad_vec')) else
              'narrow' if 'narrow' in kernel else 'f32' if 'f32q' in kernel else 'b16')
    CASES.append(dict(id=cid, dtype=dtype, shape=shape, xoff=xoff, gyoff=gyoff, gb_null=gb_null,
                      kernel=kernel % _t(dtype) if '%s' in kernel else kernel, family=family, reaches=reaches))


def _both(cid, shape, kernel, reaches):
    _case(cid + 'f', F32, shape, kernel, reaches)
    _case(cid + 'b', BF16, shape, kernel, reaches)


# ---- the general family (wgrad_plan: whatever the others turn down) ----
_both('G1', (300, 32, 32), VEC_S, 'smallest vectorised form')
_case('G2f', F32, (300, 64, 32), VEC_L, 'nct == 4: the shared-B branch, TMAX 16')
_case('G2b', BF16, (300, 64, 32), VEC_S, 'nct == 4: the shared-B branch, TMAX 4')
_case('G3', F32, (2047, 64, 64), VEC_L, 'one row under the f32 family (Q1 is the row above)')
_case('G4', BF16, (300, 192, 64), VEC_L, 'the LDPC 192 -> 64 map: 73 728 B of LDS, the attribute path')
_both('G5', (300, 128, 32), VEC_L, 'LDS exactly 48 KB, 10 chunks per thread: the WV_MAXCH boundary')
_both('G6', (300, 132, 32), SCALAR, 'just past it (f32: the chunk budget; bf16: Cin % 8)')
_case('G7', BF16, (300, 32, 256), VEC_L, 'oc = 256: brstep = 1')
_case('G8a', F32, (300, 4, 64), VEC_L, 'xpr == 1: no magic division for x')
_case('G8b', F32, (300, 64, 4), VEC_L, 'gpr == 1: no magic division for gy')
_case('G9', BF16, (300, 32, 8), VEC_S, 'gpr == 1 in bf16')
_both('G10a', (1000, 132, 68), SCALAR, 'two channel slices, the last one 4 channels')
_both('G10b', (2100, 12, 340), SCALAR, 'two channel slices, the last one 84 channels')
_both('G11a', (100, 2, 3), SCALAR, 'oc = 4 > Cout')
_both('G11b', (300, 24, 40), SCALAR, 'oc = 64 > Cout')
_case('G11c', F32, (1029, 192, 1), SCALAR, 'oc = 1')
_case('G12', F32, (500, 1024, 16), SCALAR, 'widest Cin: 135 168 B of LDS, the attribute path')
_case('G13', BF16, (2117, 1024, 256), SCALAR, '16 slices, 128 rows per workgroup (several tiles), the last one 69')
_case('G14', BF16, (8263, 192, 256), VEC_L, '4 slices, last workgroup 64 + 7 rows: the prefetch of a second, partial tile')
_case('G15a', F32, (32841, 8, 64), VEC_L, 'the synthetic-PGM input-map class: 128 rows per workgroup, the last 64 + 9')
_case('G15b', F32, (32841, 8, 32), VEC_S, 'the same in the small register tiling')
_case('G15c', BF16, (32841, 8, 32), VEC_S, 'the same in bf16')
_case('G16', F32, (2100, 64, 64), SCALAR, 'x 4 bytes off 16: f32 rule 2 -> general, scalar loads', xoff=1)
_case('G17', BF16, (300, 64, 64), SCALAR, 'x 2 bytes off: narrow rule 1, b16 rule 3 -> general, scalar loads', xoff=1)
_case('G18', F32, (2100, 64, 60), SCALAR, 'Cin Cout < 4096 at R >= 2048: f32 rule 1 -> general')

# ---- the narrow bf16 family, with gb and without; the same shapes in f32 are general-family cases ----
_NARROW = [('N1', (31, 1, 64), NARROW_X, SCALAR, 'one block of rows, Cin = 1'),
           ('N2', (1029, 2, 64), NARROW_X, SCALAR, 'the LDPC 2 -> 64 input map'),
           ('N3', (1029, 7, 256), NARROW_X, SCALAR, 'four 64-channel launches of the wide side'),
           ('N4', (33, 16, 128), NARROW_X, VEC_L, 'all 16 narrow lanes live'),
           ('N5', (1029, 64, 4), NARROW_G, VEC_L, 'the LDPC 64 -> 4 edge-type head'),
           ('N6', (1029, 256, 16), NARROW_G, SCALAR, 'four launches over x, the bias once'),
           ('N7', (1029, 192, 1), NARROW_G, None, 'Cout = 1 (f32: G11c)'),
           ('N8', (270000, 2, 64), NARROW_X, SCALAR, 'grid cap 256: more than two 32-row blocks per wave')]
for _id, _shape, _k16, _k32, _why in _NARROW:
    _case(_id, BF16, _shape, _k16, _why)
    _case(_id + 'n', BF16, _shape, _k16, _why + ', gb NULL', gb_null=True)
    if _k32:
        _case(_id + 'f', F32, _shape, _k32, 'the narrow shape in f32: ' + _why)

# ---- the f32 piece form: R = 2085 leaves a last chunk of 32 + 5 rows ----
_case('Q1', F32, (2048, 64, 64), PIECE % (64, 64), 'the first row count the family takes')
_case('Q2', F32, (2085, 132, 64), PIECE % (64, 128), 'two partially filled c blocks')
_case('Q2n', F32, (2085, 132, 64), PIECE % (64, 128), 'want_bias = 0', gb_null=True)
_case('Q3', F32, (2100, 16, 256), PIECE % (128, 64), 'the Cin Cout = 4096 edge')
_case('Q4', F32, (2100, 20, 1024), PIECE % (128, 64), 'eight o blocks, a c block of 20')
_case('Q5', F32, (2085, 1024, 1024), PIECE % (128, 128), '64 blocks, 7 slabs of 4 MB')

# ---- the bf16 family, one map ----
_case('B1', BF16, (1, 64, 64), DIRECT % 1, 'one row')
_case('B2', BF16, (300, 64, 64), DIRECT % 1, '16 row-waves')
_case('B3', BF16, (300, 64, 128), DIRECT % 2, 'two o slices')
_case('B4', BF16, (300, 128, 128), DIRECT % 4, 'o and c slices')
_case('B5', BF16, (300, 128, 256), DIRECT % 8, 'eight slices under 2048 rows: register-direct')
_case('B6', BF16, (300, 256, 256), DIRECT % 16, 'one row-wave per slice: no LDS fold')
_case('B7', BF16, (2085, 128, 256), STAGED % 8, 'LDS-staged, 64-row stages, a partial last stage')
_case('B8', BF16, (2085, 256, 256), STAGED % 16, 'LDS-staged, 32-row stages')
_case('B9', BF16, (2085, 128, 256), DIRECT % 8, 'x 8 bytes off 16: register-direct at the staged shape', xoff=4)

BY_ID = {c['id']: c for c in CASES}
assert len(BY_ID) == len(CASES)
REFUSED = [(F32, (500, 1025, 16)), (BF16, (500, 1025, 16))]      # wider than the register tiling: "" and FGNN_EUNSUPPORTED

EXACT_SETS = {F32: ('ints', 'p12', 'p20x', 'p20g'), BF16: ('ints',)}
GW0, GB0 = 1.0, 2.0                     # what gW / gb hold before the call: the entry point accumulates
LIMIT = 2 ** 24


def data_sets(case):
    return EXACT_SETS[case['dtype']] + ('rand',)


def rows_per_workgroup(case):
    """Rows of one workgroup of the f32 kernels, as wgrad_plan / fgnn_wgrad_f32_plan compute them today (the piece sets place their
    non-zero rows by it; a different split only moves those rows off the tile edges, it cannot make a set inexact)."""
    R, cin, cout = case['shape']
    if case['family'] == 'f32':
        target = max(1, 256 // (((cout + 127) // 128) * ((cin + 127) // 128)))
        rows = max(64, -(-R // target))
        return -(-rows // 32) * 32
    oc = 1
    while oc < cout and oc < 256:
        oc *= 2
    cip = -(-cin // 16)
    while oc > 16 and -(-oc // 16) * cip > 64:
        oc //= 2
    ny = -(-cout // oc)
    g = 1 if ny > 512 else 512 // ny
    return -(-max(64, -(-R // g)) // 64) * 64


def edge_rows(case):
    """Row 0, row R - 1, and rows 31, 32, 63, 64 of the last and of the first workgroup's range (inside R, without repeats)."""
    R = case['shape'][0]
    rpw = rows_per_workgroup(case)
    last = (R - 1) // rpw * rpw
    rows = [0, R - 1] + [last + d for d in (31, 32, 63, 64)] + [31, 32, 63, 64]
    out = []
    for r in rows:
        if 0 <= r < R and r not in out:
            out.append(r)
    return out


def _gen(case, name):
    return torch.Generator().manual_seed(zlib.crc32(('%s/%s' % (case['id'], name)).encode()))


def _odd(shape, bits, g, signed):
    v = (torch.randint(0, 2 ** (bits - 1), shape, generator=g) * 2 + 1).double()
    return v * (torch.randint(0, 2, shape, generator=g) * 2 - 1).double() if signed else v


def _pow2(shape, g):
    return (2.0 ** torch.randint(0, 4, shape, generator=g).double()) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()


def _one_row_per_column(case, values, g):
    R, _, cout = case['shape']
    rows = torch.randint(0, R, (cout,), generator=g)
    edges = edge_rows(case)[:cout]
    rows[:len(edges)] = torch.tensor(edges)
    gy = torch.zeros(R, cout, dtype=torch.float64)
    gy[rows, torch.arange(cout)] = values
    return gy


def make(case, name):
    """(x [R, Cin], gy [R, Cout]) of a data set, on the CPU, in the case's storage type; the same tensors on every call."""
    R, cin, cout = case['shape']
    g = _gen(case, name)
    dt = DTYPE[case['dtype']]
    if name == 'ints':
        x, gy = (torch.randint(-3, 4, (R, c), generator=g).double() for c in (cin, cout))
    elif name == 'rand':
        x, gy = (torch.randn(R, c, generator=g) for c in (cin, cout))
    elif name == 'p12':
        x, gy = _odd((R, cin), 12, g, True), _one_row_per_column(case, _odd((cout,), 12, g, False), g)
    elif name == 'p20x':
        x, gy = _odd((R, cin), 20, g, True), _one_row_per_column(case, _pow2((cout,), g), g)
    elif name == 'p20g':
        x, gy = _pow2((R, cin), g), _one_row_per_column(case, _odd((cout,), 20, g, True), g)
    else:
        raise KeyError(name)
    return x.to(dt), gy.to(dt)


def reference(x, gy):
    """(gW [Cout, Cin], gb [Cout]) in float64, on the operands' device."""
    return gy.double().t() @ x.double(), gy.double().sum(0)


def rand_bound(case, ref):
    """The project's bound for these entry points (tests/test_mpconv_gpu.py): 2e-5 of the reference's range, + 1e-5 in bf16."""
    return 2e-5 * float(ref.abs().max()) + (1e-5 if case['dtype'] == BF16 else 0.0)


def pieces(v):
    """h, m, l of an f32 tensor as the piece form cuts it: round to bf16 (nearest even), subtract, repeat."""
    out = []
    for _ in range(3):
        p = v.to(torch.bfloat16).float()
        out.append(p)
        v = v - p
    return out, v
