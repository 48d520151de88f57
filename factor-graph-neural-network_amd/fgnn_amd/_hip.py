"""ctypes binding of libfgnn_hip.so (C ABI declared in include/fgnn_hip.h).

PyTorch is only the owner of device memory and streams here: every call passes raw
device pointers, element strides and the current HIP stream.  There is no CPU or
eager-PyTorch fallback: if the shared library is missing the import of the operator
fails loudly (build it with ``python __graft_entry__.py`` or ``make -C csrc``).

The header is the one place where the interface is written down: the prototypes' ctypes signatures, the list of
exports and every mirrored constant are parsed from it when this module is imported (``signatures``, ``constants``).
Entry points added beside it live in companion headers (``bind_header``: include/fgnn_hip_ldpc_train.h,
include/fgnn_hip_pgm_bp.h, include/fgnn_hip_ldpc_code.h, include/fgnn_hip_ldpc_llr.h, include/fgnn_hip_ldpc_nms.h, include/fgnn_hip_ldpc_nms_layered.h, include/fgnn_hip_ldpc_osd.h, include/fgnn_hip_ldpc_lp.h, include/fgnn_hip_wgrad.h); ``SIGNATURES``,
``EXPORTS`` and ``ABI_VERSION`` stay the main header's.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('FGNN_HIP_LIB') or os.path.join(_HERE, 'libfgnn_hip.so')      # FGNN_HIP_LIB: a tuning build
HEADER_PATH = os.path.normpath(os.path.join(_HERE, '..', '..', 'include', 'fgnn_hip.h'))


class FgnnHipError(RuntimeError):
    pass


class MPConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ('B', 'nin', 'nou', 'net', 'N', 'M', 'k', 'ext', 'agg', 'dtype', 'relu', 'reserved')] + \
               [(n, ctypes.c_int64) for n in
                ('x_sb', 'x_sc', 'x_sn', 'idx_sb', 'idx_sm', 'idx_sk',
                 'et_sb', 'et_se', 'et_sm', 'et_sk', 'y_sb', 'y_sc', 'y_sm')]


class BnFinal(ctypes.Structure):
    """include/fgnn_hip.h: fgnn_bn_final — what a statistics-producing launch finalises in its last workgroup."""
    _fields_ = [(n, ctypes.c_void_p) for n in ('gamma', 'beta', 'running_mean', 'running_var', 'num_batches_tracked',
                                               'mean', 'invstd', 'scale', 'shift', 'shift_k')] + \
               [('count', ctypes.c_int64), ('population', ctypes.c_int64), ('momentum', ctypes.c_float), ('eps', ctypes.c_float)]


class DevicePointer:
    """``argtypes`` entry of every pointer parameter and of fgnn_stream_t: a launch site hands over the tensor itself.  A tensor
    must live on the device (no call site of this package passes host memory as a tensor; host arrays go as ctypes arrays)."""

    @classmethod
    def from_param(cls, obj):
        if isinstance(obj, torch.Tensor):
            if not obj.is_cuda:
                raise FgnnHipError('a %s tensor of shape %s was passed where libfgnn_hip expects device memory'
                                   % (obj.device, tuple(obj.shape)))
            return ctypes.c_void_p(obj.data_ptr())
        if obj is None or isinstance(obj, (ctypes.c_void_p, ctypes.Array, ctypes._Pointer)):
            return obj
        if isinstance(obj, int):
            return ctypes.c_void_p(obj)
        raise TypeError('expected a tensor, None, an address or a ctypes array / pointer, got %s' % type(obj).__name__)


_SCALARS = {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64,
            'float': ctypes.c_float, 'double': ctypes.c_double, 'fgnn_stream_t': DevicePointer}
_STRUCTS = {'fgnn_mpconv_desc': MPConvDesc, 'fgnn_bn_final': BnFinal}


def _uncommented(header_text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', header_text, flags=re.S))


def _ctype(decl, proto, returned=False):
    """ctypes type of one C type as the header spells it (``int64_t``, ``const float* const*``, ...); unknown: FgnnHipError."""
    words = [w for w in decl.replace('*', ' * ').split() if w != 'const']
    if words and re.fullmatch(r'\w+', words[0]) and all(w == '*' for w in words[1:]):
        base, depth = words[0], len(words) - 1
        if depth == 0 and base in _SCALARS:
            return _SCALARS[base]
        if returned:
            if words == ['void']:
                return None
            if words == ['char', '*']:
                return ctypes.c_char_p
        elif depth == 1 and base in _STRUCTS:
            return ctypes.POINTER(_STRUCTS[base])
        elif depth >= 1:
            return DevicePointer
    raise FgnnHipError('include/fgnn_hip.h: no ctypes type for `%s` in `%s`' % (decl.strip(), proto))


def signatures(header_text):
    """{name: (restype, [(parameter name, argtype), ...])} of every fgnn_* prototype at file scope of the header.  Pure text
    work (no library, no GPU).  A declaration that does not split into a prototype, or a type outside the map, raises."""
    text = re.sub(r'^[ \t]*#.*$', '', _uncommented(header_text), flags=re.M).replace('extern "C" {', '')
    text = re.sub(r'\{[^{}]*\}', '', text)                              # struct and enum bodies
    out = {}
    for stmt in text.split(';'):
        stmt = ' '.join(stmt.split())
        if not stmt or stmt == '}' or stmt.startswith(('typedef ', 'enum')):
            continue
        m = re.fullmatch(r'(.*?)\b(fgnn_\w+) ?\((.*)\)', stmt)
        if not m:
            raise FgnnHipError('include/fgnn_hip.h: cannot parse the declaration `%s`' % stmt)
        ret, name, plist = m.groups()
        params = []
        for p in [] if plist.strip() == 'void' else plist.split(','):
            pm = re.fullmatch(r'(.*\W)(\w+)', p.strip())
            if not pm:
                raise FgnnHipError('include/fgnn_hip.h: cannot parse the parameter `%s` of `%s`' % (p.strip(), stmt))
            params.append((pm.group(2), _ctype(pm.group(1), stmt)))
        out[name] = (_ctype(ret, stmt, returned=True), params)
    return out


def constants(header_text):
    """{name without FGNN_: value} of the header's enum members and of its #defines that have a value."""
    text = _uncommented(header_text)
    pairs = re.findall(r'^[ \t]*#define[ \t]+FGNN_(\w+)[ \t]+(\S.*)$', text, flags=re.M)
    for body in re.findall(r'\benum\s*\{([^}]*)\}', text):
        pairs += re.findall(r'FGNN_(\w+)\s*=\s*([^,]+)', body)
    out = {}
    for name, value in pairs:
        if not re.fullmatch(r'[\s\dxXa-fA-F()+*-]+', value):
            raise FgnnHipError('include/fgnn_hip.h: FGNN_%s = `%s` is not an integer expression' % (name, value.strip()))
        out[name] = int(eval(value, {'__builtins__': {}}))              # digits, parentheses, + - * only (checked above)
    return out


def _header():
    if not os.path.exists(HEADER_PATH):
        raise FgnnHipError('the C-ABI header was not found at %s — the binding is derived from it and has no built-in '
                           'copy of the interface' % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return f.read()


SIGNATURES, _K = (parse(_header()) for parse in (signatures, constants))
EXPORTS = tuple(SIGNATURES)
EXT_NONE, EXT_NEIGHBOR, EXT_DIFF = _K['EXT_NONE'], _K['EXT_NEIGHBOR'], _K['EXT_DIFF']
DESC_GETYPE_REDUCED = _K['DESC_GETYPE_REDUCED']
DESC_IDENTITY_LIST = _K['DESC_IDENTITY_LIST']       # forward: the one-destination call's neighbour table is idx[j] == j
AGG_MAX, AGG_LSE, AGG_MEAN = _K['AGG_MAX'], _K['AGG_LSE'], _K['AGG_MEAN']
F32, BF16 = _K['F32'], _K['BF16']
DEC_F32, DEC_BF16, DEC_U8 = _K['DEC_F32'], _K['DEC_BF16'], _K['DEC_U8']              # fgnn_ldpc_error_counts
LABEL_I64, LABEL_U8 = _K['LABEL_I64'], _K['LABEL_U8']
PGM_DEC_F32, PGM_DEC_BF16, PGM_DEC_I64 = _K['PGM_DEC_F32'], _K['PGM_DEC_BF16'], _K['PGM_DEC_I64']   # fgnn_chain_budget_score
ABI_VERSION = _K['ABI_VERSION']             # checked before any symbol is bound
EUNSUPPORTED = _K['EUNSUPPORTED']           # shape outside a kernel's family (callers fall back)
FOLD_SCRATCH_BYTES = _K['FOLD_SCRATCH_BYTES']

AGG_CODES = {'max': AGG_MAX, 'softmax': AGG_LSE, 'mean': AGG_MEAN}


def bn_final(stats, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, count, population=0):
    """fgnn_bn_final for a BatchNorm whose outputs go to ``stats`` [4, C] f32 (rows: mean, invstd, scale, shift).  The caller keeps
    the tensors alive until the launch is enqueued."""
    f = BnFinal()
    dp = lambda t: None if t is None else t.data_ptr()
    f.gamma, f.beta = dp(gamma), dp(beta)
    f.running_mean, f.running_var, f.num_batches_tracked = dp(running_mean), dp(running_var), dp(num_batches_tracked)
    f.mean, f.invstd, f.scale, f.shift = (stats[i].data_ptr() for i in range(4))
    f.shift_k = None
    f.count, f.population = int(count), int(population)
    f.momentum, f.eps = float(momentum), float(eps)
    return f


_lib = None
COMPANIONS = {}     # {name: (restype, [(parameter name, argtype), ...])} of the companion headers bound so far (bind_header)
_MISSING = {}       # {companion name: header file} the loaded library does not export (a build from before that header)


def _bind_companions(L, sigs, header):
    for name, (restype, params) in sigs.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            _MISSING[name] = header
            continue
        fn.restype, fn.argtypes = restype, [t for _, t in params]
        _MISSING.pop(name, None)


def bind_header(path):
    """Bind the prototypes of a companion header (a file beside include/fgnn_hip.h that includes it and declares further entry
    points in the same style): parsed by ``signatures``, given ``restype`` / ``argtypes`` on the library (now if it is loaded, else
    when ``lib()`` loads it) and resolved by ``invoke`` / ``call`` like the main header's names, with the same argument-count check
    and stream default.  ``SIGNATURES`` / ``EXPORTS`` are not extended.  A library without one of the symbols still loads; calling
    that name raises FgnnHipError.  Returns the tuple of names."""
    if not os.path.isabs(path):
        path = os.path.join(os.path.dirname(HEADER_PATH), path)
    if not os.path.exists(path):
        raise FgnnHipError('the companion header %s was not found' % path)
    with open(path) as f:
        sigs = signatures(f.read())
    clash = sorted(set(sigs) & set(SIGNATURES))
    if clash:
        raise FgnnHipError('%s declares %s again (include/fgnn_hip.h has it)' % (os.path.basename(path), ', '.join(clash)))
    for name in sigs:
        COMPANIONS[name] = sigs[name] + (os.path.basename(path),)
    if _lib is not None:
        _bind_companions(_lib, sigs, os.path.basename(path))
    return tuple(sigs)


def _prototype(name):
    """(restype, params) of a main-header or companion name."""
    if name in SIGNATURES:
        return SIGNATURES[name]
    return COMPANIONS[name][:2]          # (a name in neither table: KeyError, as before companions existed)


def _entry(name):
    """The bound function; a companion name the loaded library lacks raises FgnnHipError (never AttributeError)."""
    L = lib()
    if name in _MISSING:
        raise FgnnHipError('%s does not export %s (include/%s): it was built before that header — rebuild it with '
                           '`python __graft_entry__.py`' % (LIB_PATH, name, _MISSING[name]))
    return getattr(L, name)


def lib():
    """Load libfgnn_hip.so once; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FgnnHipError(
            'libfgnn_hip.so not found at %s — the FGNN message operator has no CPU/eager '
            'fallback; build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950).'
            % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    try:
        L.fgnn_abi_version.restype = ctypes.c_int
        have = int(L.fgnn_abi_version())
    except AttributeError:
        have = None
    if have != ABI_VERSION:
        raise FgnnHipError('%s speaks C-ABI version %s, this package binds version %d (include/fgnn_hip.h): rebuild it '
                           'with `python __graft_entry__.py`' % (LIB_PATH, have, ABI_VERSION))
    for name, (restype, params) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, [t for _, t in params]
    for header in sorted({c[2] for c in COMPANIONS.values()}):
        _bind_companions(L, {n: c[:2] for n, c in COMPANIONS.items() if c[2] == header}, header)
    _lib = L
    return L


def invoke(name, *args):
    """The entry point ``name`` with the prototype's arguments, exactly (ctypes itself lets extra ones through): tensors go as they
    are (``DevicePointer``), and a prototype that ends in ``stream`` may be called without it and then runs on torch's current
    stream.  Returns what the entry point returns.  Tensors stay the caller's to keep alive until this returns."""
    params = _prototype(name)[1]
    if len(args) == len(params) - 1 and params[-1][0] == 'stream':
        args += (stream_ptr(),)
    if len(args) != len(params):
        raise TypeError('%s takes %d arguments (%s), got %d' % (name, len(params), ', '.join(n for n, _ in params), len(args)))
    try:
        return _entry(name)(*args)
    except ctypes.ArgumentError as e:       # (ctypes' wrapper around what an argtype's from_param raised, e.g. for a host tensor)
        raise FgnnHipError('%s: %s' % (name, e)) from None


def call(name, *args):
    """``invoke`` for a launch, i.e. an entry point whose int return is a status: a non-zero status raises.  (A site that
    branches on the status, such as on EUNSUPPORTED, uses ``invoke``; the size / support queries call ``lib()`` directly.)"""
    check(invoke(name, *args))


def check(rc):
    if rc != 0:
        raise FgnnHipError('libfgnn_hip: %s (code %d)' % (lib().fgnn_last_error().decode(), rc))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise FgnnHipError('fgnn_amd supports float32 and bfloat16 tensors, got %s' % t.dtype)


def make_desc(x, nn_idx, etype, nou, net, ext, agg, relu, y=None):
    """Describe one operator call from tensor views (no copies).

    x [B,nin,N,1] (any strides), nn_idx [B,M,k] int64, etype [B,net,M,k].  A batch
    stride of 0 (``expand``-ed tensors) marks a graph / edge weights shared by the batch.
    """
    B, nin, N = x.shape[0], x.shape[1], x.shape[2]
    M, k = nn_idx.shape[1], nn_idx.shape[2]
    d = MPConvDesc()
    d.B, d.nin, d.nou, d.net, d.N, d.M, d.k = B, nin, nou, net, N, M, k
    d.ext, d.agg, d.dtype, d.relu = ext, agg, dtype_code(x), int(bool(relu))
    d.x_sb, d.x_sc, d.x_sn = x.stride(0), x.stride(1), x.stride(2)
    d.idx_sb, d.idx_sm, d.idx_sk = nn_idx.stride(0), nn_idx.stride(1), nn_idx.stride(2)
    d.et_sb, d.et_se, d.et_sm, d.et_sk = (etype.stride(0), etype.stride(1),
                                          etype.stride(2), etype.stride(3))
    if y is not None:
        d.y_sb, d.y_sc, d.y_sm = y.stride(0), y.stride(1), y.stride(2)
    return d


LDPC_TRAIN = bind_header('fgnn_hip_ldpc_train.h')      # fgnn_ldpc_sample_rng, fgnn_ldpc_loss_parts_forward
PGM_BP = bind_header('fgnn_hip_pgm_bp.h')              # fgnn_chain_budget_bp, fgnn_chain_budget_bp_lds_bytes
LDPC_CODE = bind_header('fgnn_hip_ldpc_code.h')        # fgnn_ldpc_encode_words, fgnn_ldpc_sample_rng_words
LDPC_LLR = bind_header('fgnn_hip_ldpc_llr.h')          # fgnn_ldpc_decode_llr, fgnn_ldpc_decode_llr_lds_bytes
LDPC_NMS = bind_header('fgnn_hip_ldpc_nms.h')          # fgnn_ldpc_nms_forward, _backward and their four size queries
LDPC_NMS_LAYERED = bind_header('fgnn_hip_ldpc_nms_layered.h')     # fgnn_ldpc_nms_layered_forward, _backward, _lds_bytes
LDPC_OSD = bind_header('fgnn_hip_ldpc_osd.h')          # fgnn_ldpc_osd, fgnn_ldpc_osd_lds_bytes
LDPC_LP = bind_header('fgnn_hip_ldpc_lp.h')            # fgnn_ldpc_decode_lp, fgnn_ldpc_decode_lp_lds_bytes
WGRAD = bind_header('fgnn_hip_wgrad.h')                # fgnn_linear_wgrad_kernel: the kernel a weight-gradient call would run
