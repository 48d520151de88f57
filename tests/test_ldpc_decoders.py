"""CPU: the decoder modules import in any order, and none reaches into a sibling for a private name (fgnn_amd/ldpc_decoders.py,
datapath.py, ldpc_nms.py, ldpc_eval.py)."""
import ast
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'factor-graph-neural-network_amd')
MODULES = ('ldpc_decoders', 'datapath', 'ldpc_nms', 'ldpc_eval')


@pytest.mark.parametrize('first', MODULES)
def test_the_modules_import_in_every_order(first):
    """A fresh interpreter per order (the six orders that begin with ``first``), so no earlier import hides a cycle."""
    orders = [o for o in itertools.permutations(MODULES) if o[0] == first]
    procs = [subprocess.Popen([sys.executable, '-c', 'import sys; sys.path.insert(0, %r)\n' % PKG
                               + ''.join('import fgnn_amd.%s\n' % m for m in order)], stderr=subprocess.PIPE, text=True)
             for order in orders]
    for order, p in zip(orders, procs):
        err = p.communicate()[1]
        assert p.returncode == 0, (order, err)


def test_no_module_imports_a_private_name_from_a_sibling():
    for module in MODULES:
        tree = ast.parse(open(os.path.join(PKG, 'fgnn_amd', module + '.py')).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level >= 1 and node.module:        # from .sibling import names
                private = [a.name for a in node.names if a.name.startswith('_')]
                assert not private, '%s.py imports %s from .%s' % (module, private, node.module)


def test_the_decoders_live_in_the_base_class_and_a_decoder_is_still_a_triple():
    from fgnn_amd import datapath, ldpc_decoders, ldpc_eval
    for name in ('decode', 'decode_llr', 'decode_osd', 'bit_prior', 'bit_llr'):            # no forwarding stubs
        assert name not in vars(datapath.LdpcDataPath) and name in vars(ldpc_decoders.LdpcDecoders)
    assert ldpc_eval.parse_decoder is ldpc_decoders.parse_decoder and ldpc_eval.LdpcDataPath is datapath.LdpcDataPath
    d = ldpc_decoders.parse_decoder('mackay:iters=20')
    canon, kind, kw = d
    assert (d.spec, d.kind, d.args) == (canon, kind, kw) == ('mackay:iters=20', 'mackay', {'loops': 20})
