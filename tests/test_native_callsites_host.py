"""CPU: every ``<something>.dsgcn_*(...)`` call in the package, the tools, the tests and bench.py names an entry point that
``native.SIGNATURES`` (or ``LAB_SIGNATURES``) binds, and passes as many positional arguments as its argtypes — a stale
caller of a removed or changed entry point shows here, without a GPU.  Calls with a starred argument are only checked by
name."""
import ast
import glob
import os

from dsgcn_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files():
    pkg = os.path.dirname(os.path.abspath(native.__file__))
    files = sorted(glob.glob(os.path.join(pkg, '*.py')))
    for sub in ('tools', 'tests'):
        files += sorted(glob.glob(os.path.join(ROOT, sub, '*.py')))
    return files + [os.path.join(ROOT, 'bench.py')]


def test_native_call_sites_match_the_bindings():
    known = {**native.SIGNATURES, **native.LAB_SIGNATURES}
    plain = starred = 0
    bad = []
    for path in _files():
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                    and node.func.attr.startswith('dsgcn_')):
                continue
            name, where = node.func.attr, f'{os.path.relpath(path, ROOT)}:{node.lineno}'
            if name not in known:
                bad.append(f'{where}: {name} is not bound')
            elif any(isinstance(a, ast.Starred) for a in node.args):
                starred += 1
                continue
            elif len(node.args) != len(known[name]) or node.keywords:
                bad.append(f'{where}: {name} takes {len(known[name])} arguments, called with {len(node.args)}')
            plain += 1
    assert not bad, '\n'.join(bad)
    # the test must not pass by finding nothing
    assert plain >= 400, plain
    assert starred <= 0.15 * (plain + starred), (starred, plain)
