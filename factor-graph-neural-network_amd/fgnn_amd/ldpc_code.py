"""``LdpcCode`` — one immutable description of a REGULAR LDPC code for the data path, the sum-product baseline and the decoder model.

Host side, numpy, no device.  The reference is locked to MacKay's 96.3.963 (/root/reference/lib/data/ldpc_dataset.py:11-106: the alist
file, 96 / 48 and the generator file are written into the code); ``LdpcCode.builtin()`` is that code with the packaged tables, and the
other constructors describe any code in which every variable sits in ``dv`` checks and every check touches ``dc`` variables — the
model's neighbour tables have one width, so an irregular H is refused.

Generator.  GF(2) Gauss-Jordan elimination of H [M, N] with column pivoting, rows packed into 64-bit words.  The pivot rule is fixed, so
``(n, dv, dc, seed)`` names one code: columns are scanned from the LAST to the first; a column becomes a pivot if a row not yet used
has a one in it (the first such row, in the current row order); it is then cleared from every other row.  ``P = rank(H)`` pivots are
found (redundant checks lower P below M: Gallager codes with dv = 3 lose 2); ``K = N - P``.  The variables are relabelled so that the K
non-pivot columns come first (in their original order) and the P pivot columns last (in increasing original order): ``perm[i]`` is the
original index of position i, ``H`` is the input's ``H[:, perm]`` with ALL M checks kept, and ``codeword = [s | G s mod 2]`` with
``G`` [P, K], as for the built-in code.

Limits (``ValueError`` names the one hit): N <= 1024 for the data path (the feature kernels' LDS row), checked on construction;
N * dv <= 1024 and degrees <= 16 for the sum-product baseline (``require_decoder``); N <= 1024, M <= 1024 and degrees <= 16 for the
LLR-domain decoders (``require_llr_decoder``: min-sum, offset min-sum, sum-product; csrc/ldpc_llr.hip); N <= 132 for the model (``require_model``); dv = 3,
dc = 6 and N <= 96 for the training loop (``require_trainer``).  The operator itself takes a hyper-factor of up to 255 variables; the
last two limits are narrower than that on purpose: they are the sizes at which the model's forward and backward, and training at any
batch, have run on the device against the oracle — the trainer's is the shape class whose bf16 calls fall to the kernel families the
built-in code trains on.  A code inside the first limit but outside a later one is still usable for what it fits.
"""
import os

import numpy as np

from .tables import _DATA

MAX_VAR = 1024              # csrc/ldpc_datapath.hip, csrc/ldpc_code.hip: the feature kernels' LDS row
DEC_MAXE, DEC_MAXD = 1024, 16       # csrc/ldpc_decode.hip
LLR_MAXV, LLR_MAXD = 1024, 16       # csrc/ldpc_word.h's LDPC_MAXV, LDPC_MAXD: variables / checks, edges per variable / check
MODEL_MAX_VAR = 132         # the model: verified up to here (the message operator's own bound is k <= 255)
TRAIN_MAX_VAR, TRAIN_DV, TRAIN_DC = 96, 3, 6      # the training loop: the built-in code's shape class


def _check_parity_matrix(H):
    """The limits every constructor applies to H [M, N] uint8: the data path's N and regularity.  Returns (dv, dc)."""
    M, N = H.shape
    if N > MAX_VAR:
        raise ValueError('N = %d variables: the data path takes N <= %d (the feature kernels\' LDS row)' % (N, MAX_VAR))
    colw, roww = H.sum(0), H.sum(1)
    if M < 1 or N < 1 or colw.min() != colw.max() or roww.min() != roww.max() or colw[0] < 1:
            raise ValueError('irregular parity-check matrix: column weights %d..%d, row weights %d..%d; only regular codes (one dv, one dc) '
                             'are supported — the model\'s neighbour tables have one width' % (colw.min(), colw.max(), roww.min(), roww.max()))
    return int(colw[0]), int(roww[0])


def _pack_rows(A):
    """0/1 matrix [R, C] -> uint64 [R, ceil(C / 64)]: column c in bit c % 64 of word c // 64."""
    A = np.asarray(A, np.uint8)
    R, C = A.shape
    W = max(1, -(-C // 64))
    pad = np.zeros((R, W * 64), np.uint8)
    pad[:, :C] = A
    return np.packbits(pad.reshape(R, W, 64), axis=2, bitorder='little').view(np.uint64).reshape(R, W)


def _unpack_rows(words, C):
    R = words.shape[0]
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(R, -1), axis=1, bitorder='little')[:, :C]


def _eliminate(H):
    """Gauss-Jordan over GF(2) by the module's pivot rule.  Returns (reduced rows [rank, N] uint8 in pivot order, pivot columns)."""
    M, N = H.shape
    rows = _pack_rows(H)
    pivots, r = [], 0
    for col in range(N - 1, -1, -1):
        if r == M:
            break
        w, bit = col // 64, np.uint64(1) << np.uint64(col % 64)
        has = np.nonzero(rows[r:, w] & bit)[0]
        if has.size == 0:
            continue
        i = r + int(has[0])
        if i != r:
            rows[[r, i]] = rows[[i, r]]
        others = np.nonzero(rows[:, w] & bit)[0]
        others = others[others != r]
        rows[others] ^= rows[r]
        pivots.append(col)
        r += 1
    return _unpack_rows(rows[:r], N), pivots


class LdpcCode:
    """See the module docstring.  Attributes: n_var, n_chk, dv, dc, K, P, G [P, K] uint8, H [M, N] uint8 (relabelled), perm [N] int64,
    var_to_factors [N, dv] int64, factor_to_vars [M, dc] int64, nlist (each variable's checks in alist order, -1 = padding: what
    ``oracle.ldpc_sum_product`` and ``LdpcDataPath.decode`` read), is_default (the packaged 96.3.963 tables)."""


    def __init__(self, H, G, perm, var_to_factors=None, factor_to_vars=None, nlist=None, is_default=False):
        H = np.ascontiguousarray(H, np.uint8)
        M, N = H.shape
        dv, dc = _check_parity_matrix(H)
        G = np.ascontiguousarray(G, np.uint8)
        P, K = G.shape
        if K < 1 or K + P != N:
            raise ValueError('G [P = %d, K = %d] does not fit N = %d variables with at least one message bit' % (P, K, N))
        if var_to_factors is None:
            var_to_factors = np.nonzero(H.T)[1].reshape(N, dv)            # each variable's checks, increasing
        if factor_to_vars is None:
            factor_to_vars = np.nonzero(H)[1].reshape(M, dc)              # each check's variables, increasing
        if nlist is None:
            nlist = np.asarray(var_to_factors, np.int32)
        vals = dict(n_var=N, n_chk=M, dv=dv, dc=dc, K=int(K), P=int(P), G=G, H=H, perm=np.ascontiguousarray(perm, np.int64),
                    var_to_factors=np.ascontiguousarray(var_to_factors, np.int64),
                    factor_to_vars=np.ascontiguousarray(factor_to_vars, np.int64), nlist=np.ascontiguousarray(nlist, np.int32),
                    is_default=bool(is_default))
        for k, v in vals.items():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError('LdpcCode is immutable')

    def __repr__(self):
        return 'LdpcCode(N=%d, M=%d, dv=%d, dc=%d, K=%d, P=%d%s)' % (self.n_var, self.n_chk, self.dv, self.dc, self.K, self.P,
                                                                      ', builtin' if self.is_default else '')

    # ---- constructors ---------------------------------------------------------------------------------------------------------------

    @classmethod
    def builtin(cls):
        """The packaged 96.3.963 with exactly the packaged tables, in their order, its G and its variable order."""
        z = np.load(os.path.join(_DATA, 'ldpc_96_3_963.npz'))
        g = np.load(os.path.join(_DATA, 'ldpc_96_3_963_G.npz'))
        v2f, f2v = z['var_to_factors'].astype(np.int64), z['factor_to_vars'].astype(np.int64)
        H = np.zeros((f2v.shape[0], v2f.shape[0]), np.uint8)
        for m in range(f2v.shape[0]):
            H[m, f2v[m]] = 1
        return cls(H, g['G'], np.arange(v2f.shape[0]), v2f, f2v, g['A2_nlist'], is_default=True)

    @classmethod
    def from_parity_check(cls, H):
        """H [M, N] of 0/1: the generator by the module's elimination, the variables relabelled (message positions first)."""
        H = np.asarray(H)
        if H.ndim != 2 or H.size == 0 or not np.isin(H, (0, 1)).all():
            raise ValueError('H must be a non-empty [M, N] matrix of 0 / 1')
        H = H.astype(np.uint8)
        N = H.shape[1]
        _check_parity_matrix(H)
        red, pivots = _eliminate(H)
        pivots = np.asarray(pivots, np.int64)
        order = np.argsort(pivots)                                  # parity positions in increasing original order
        is_pivot = np.zeros(N, bool)
        is_pivot[pivots] = True
        msg = np.nonzero(~is_pivot)[0]
        perm = np.concatenate([msg, pivots[order]])
        return cls(H[:, perm], red[order][:, msg], perm)

    @classmethod
    def gallager(cls, n_var, dv, dc, seed):
        """Gallager's band construction: ``dv`` bands of ``n_var / dc`` checks, each variable once per band.  Band 0 takes consecutive
        variables; band b > 0 takes ``numpy.random.RandomState(seed).permutation(n_var)``, drawn in order of b."""
        n_var, dv, dc = int(n_var), int(dv), int(dc)
        if n_var < 1 or dv < 1 or dc < 1 or n_var % dc:
            raise ValueError('gallager: n_var = %d must be a positive multiple of dc = %d (and dv = %d >= 1)' % (n_var, dc, dv))
        rs = np.random.RandomState(int(seed))
        per = n_var // dc
        H = np.zeros((dv * per, n_var), np.uint8)
        for b in range(dv):
            order = np.arange(n_var) if b == 0 else rs.permutation(n_var)
            H[b * per + np.arange(n_var) // dc, order] = 1
        return cls.from_parity_check(H)

    @classmethod
    def from_alist(cls, path):
        """MacKay's alist format: ``N M`` / ``max dv, max dc`` / the N column weights / the M row weights / N lines of 1-based check
        indices / M lines of 1-based variable indices (0 = padding)."""
        with open(path) as f:
            tok = [[int(t) for t in line.split()] for line in f if line.strip()]
        try:
            (N, M), colw, roww = tok[0], tok[2], tok[3]
            cols, rows = tok[4:4 + N], tok[4 + N:4 + N + M]
            if len(colw) != N or len(roww) != M or len(cols) != N or len(rows) != M:
                raise IndexError
        except (IndexError, ValueError):
            raise ValueError('%s is not an alist file (N M / max weights / column weights / row weights / N + M index lines)' % path) from None
        if N > MAX_VAR:
            _check_parity_matrix(np.zeros((1, N), np.uint8))        # (names the limit before a matrix of that size is filled)
        H = np.zeros((M, N), np.uint8)
        for n, c in enumerate(cols):
            c = [m for m in c if m != 0]
            if len(c) != colw[n] or any(not 1 <= m <= M for m in c):
                raise ValueError('%s: variable %d lists %s, weight %d, M = %d' % (path, n + 1, c, colw[n], M))
            for m in c:
                if H[m - 1, n]:
                    raise ValueError('%s: the edge (variable %d, check %d) is listed twice' % (path, n + 1, m))
                H[m - 1, n] = 1
        for m, r in enumerate(rows):
            r = [n for n in r if n != 0]
            if len(set(r)) != len(r):
                raise ValueError('%s: check %d lists a variable twice: %s' % (path, m + 1, r))
            if len(r) != roww[m] or any(not 1 <= n <= N for n in r) or any(not H[m, n - 1] for n in r) or H[m].sum() != len(r):
                raise ValueError('%s: the row list of check %d does not match the column lists' % (path, m + 1))
        return cls.from_parity_check(H)

    def to_alist(self, path):
        """``from_alist``'s inverse: this code's incidence (variables in this code's order), lists in the tables' order."""
        with open(path, 'w') as f:
            f.write('%d %d\n%d %d\n' % (self.n_var, self.n_chk, self.dv, self.dc))
            f.write(' '.join([str(self.dv)] * self.n_var) + ' \n')
            f.write(' '.join([str(self.dc)] * self.n_chk) + ' \n')
            for row in self.var_to_factors:
                f.write('\t'.join(str(int(m) + 1) for m in row) + '\n')
            for row in self.factor_to_vars:
                f.write('\t'.join(str(int(n) + 1) for n in row) + '\n')

    @classmethod
    def from_spec(cls, spec):
        """The command lines' ``--code``: ``builtin``, ``gallager:N,dv,dc,seed`` or the path of an alist file."""
        if spec is None or spec == 'builtin':
            return cls.builtin()
        if spec.startswith('gallager:'):
            try:
                n, dv, dc, seed = (int(v) for v in spec[len('gallager:'):].split(','))
            except ValueError:
                raise ValueError('--code gallager:N,dv,dc,seed takes four integers, got %r' % spec) from None
            return cls.gallager(n, dv, dc, seed)
        return cls.from_alist(spec)

    # ---- what the layers read -------------------------------------------------------------------------------------------------------

    @property
    def W(self):
        """64-bit words per packed message / row of G."""
        return -(-self.K // 64)

    @property
    def gwords(self):
        """G's rows packed over the K message bits: uint64 [P, W], bit c of a row in bit c % 64 of word c // 64 (W = 1: the one-word
        kernels' ``gmask``)."""
        return _pack_rows(self.G)

    def require_decoder(self):
        """The sum-product baseline's limits (csrc/ldpc_decode.hip: DEC_MAXE edges, DEC_MAXD per variable / check)."""
        edges = int((self.nlist >= 0).sum())
        deg = max(int((self.nlist >= 0).sum(1).max()), self.dc, self.dv)
        if edges > DEC_MAXE:
            raise ValueError('N * dv = %d edges: the sum-product decoder takes at most %d' % (edges, DEC_MAXE))
        if deg > DEC_MAXD:
            raise ValueError('degree %d: the sum-product decoder takes at most %d checks per variable / variables per check' % (deg, DEC_MAXD))
        return self

    def require_llr_decoder(self):
        """The LLR-domain decoders' limits (``LLR_MAXV`` variables and checks, ``LLR_MAXD`` per variable / check: csrc/ldpc_word.h's LDPC_MAXV, LDPC_MAXD)."""
        deg = max(int((self.nlist >= 0).sum(1).max()), self.dc, self.dv)
        if self.n_var > LLR_MAXV:
            raise ValueError('N = %d variables: the LLR-domain decoders take at most %d' % (self.n_var, LLR_MAXV))
        if self.n_chk > LLR_MAXV:
            raise ValueError('M = %d checks: the LLR-domain decoders take at most %d' % (self.n_chk, LLR_MAXV))
        if deg > LLR_MAXD:
            raise ValueError('degree %d: the LLR-domain decoders take at most %d checks per variable / variables per check' % (deg, LLR_MAXD))
        return self

    def incidence_tables(self):
        """(col_ptr [N + 1], row_ptr [M + 1], row_edge [E], row_var [E]) read-only int32, the decoders' tables (``fgnn_ldpc_decode``'s;
        csrc/ldpc_word.h): edge e = col_ptr[n] + u is variable n's u-th check in ``nlist``'s order; check m's edges are
        row_edge[row_ptr[m] .. row_ptr[m + 1] - 1], their variables row_var[..], in increasing variable order.  Memoised."""
        memo = self.__dict__.get('_incidence')
        if memo is None:
            cols = [[int(m) for m in row if m >= 0] for row in self.nlist]
            col_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
            rows = [[] for _ in range(self.n_chk)]
            for n, c in enumerate(cols):
                for u, m in enumerate(c):
                    rows[m].append((int(col_ptr[n]) + u, n))
            row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
            memo = (col_ptr, row_ptr, np.array([e for r in rows for e, _ in r], np.int32), np.array([n for r in rows for _, n in r], np.int32))
            for a in memo:
                a.setflags(write=False)
            object.__setattr__(self, '_incidence', memo)
        return memo

    def layers(self):
        """(layer_ptr [n_layers + 1], layer_chk [M]) int32: the checks partitioned into layers for a layered decoding schedule, no
        two checks of a layer sharing a variable.  Fixed greedy rule: the checks in index order, each into the first layer none of
        whose checks shares a variable with it (a Gallager code: its dv bands).  Memoised."""
        memo = self.__dict__.get('_layers')
        if memo is None:
            used, members = [], []                      # per layer: the variables taken, the checks
            rows = [[] for _ in range(self.n_chk)]      # (from nlist: the incidence the decoders' tables are built from)
            for n, col in enumerate(self.nlist):
                for m in col[col >= 0]:
                    rows[int(m)].append(n)
            for m in range(self.n_chk):
                vs = np.asarray(rows[m], np.int64)
                for k in range(len(used)):
                    if not used[k][vs].any():
                        break
                else:
                    k = len(used)
                    used.append(np.zeros(self.n_var, bool))
                    members.append([])
                used[k][vs] = True
                members[k].append(m)
            layer_ptr = np.concatenate([[0], np.cumsum([len(c) for c in members])]).astype(np.int32)
            layer_chk = np.array([m for c in members for m in c], np.int32)
            layer_ptr.setflags(write=False)
            layer_chk.setflags(write=False)
            memo = (layer_ptr, layer_chk)
            object.__setattr__(self, '_layers', memo)
        return memo

    def require_model(self):
        """The model's limit (``MODEL_MAX_VAR``)."""
        if self.n_var > MODEL_MAX_VAR:
            raise ValueError('N = %d variables: the model takes N <= %d (the largest size its forward and backward are verified at; its '
                             'hyper-factor listens to all N variables)' % (self.n_var, MODEL_MAX_VAR))
        return self

    def require_trainer(self):
        """The training loop's limits: the model's, and the built-in code's shape class (dv = 3, dc = 6, N <= 96)."""
        self.require_model()
        if (self.dv, self.dc) != (TRAIN_DV, TRAIN_DC) or self.n_var > TRAIN_MAX_VAR:
            raise ValueError('the training loop takes codes with dv = %d, dc = %d and N <= %d variables (the shape class of the kernels it '
                             'is verified on), got dv = %d, dc = %d, N = %d' % (TRAIN_DV, TRAIN_DC, TRAIN_MAX_VAR, self.dv, self.dc, self.n_var))
        return self

    def checkpoint_entry(self):
        """What a checkpoint trained for a non-default code carries under 'code' (tensors, so ``weights_only`` loading reads it)."""
        import torch
        return {'n_var': torch.tensor(self.n_var), 'n_chk': torch.tensor(self.n_chk), 'dv': torch.tensor(self.dv),
                'dc': torch.tensor(self.dc), 'var_to_factors': torch.from_numpy(self.var_to_factors.copy())}

    def check_checkpoint(self, ckpt, where='checkpoint'):
        """Refuse a checkpoint dict trained for another code (no 'code' entry: the default code's)."""
        entry = ckpt.get('code')
        if entry is None:
            same, theirs, note = self.is_default, 'the built-in 96.3.963 code', ''
        else:
            sizes = tuple(int(entry[k]) for k in ('n_var', 'n_chk', 'dv', 'dc'))
            theirs = 'a code with (N, M, dv, dc) = %s' % (sizes,)
            same_sizes = sizes == (self.n_var, self.n_chk, self.dv, self.dc)
            same = same_sizes and np.array_equal(np.asarray(entry['var_to_factors']), self.var_to_factors)
            note = ' (the same sizes but another incidence: another code)' if same_sizes else ''
        if not same:
            raise ValueError('%s was trained for %s, not for %r%s: pass the code it was trained for (--code)' % (where, theirs, self, note))
