#!/usr/bin/env python3
"""Per-kernel register / scratch / LDS figures of libdsgcn.so, read from the gfx950 code objects' metadata notes.

    python tools/codeobj_report.py [--lib PATH] [--spills] [--json] [--digest]

The library is a host ELF with one offload bundle per translation unit; ``llvm-objdump --offloading`` unpacks them (into
a temporary directory — it writes next to its input) and ``llvm-readelf --notes`` prints the AMDGPU metadata
(`.vgpr_count`, `.vgpr_spill_count`, `.private_segment_fixed_size`, `.group_segment_fixed_size` per kernel).
tests/test_native_abi.py uses ``kernels()`` to keep every kernel a BASELINE step launches free of scratch."""
import argparse
import contextlib
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
DEFAULT_LIB = os.path.join(ROOT, 'ds-gcn_amd', 'lib', 'libdsgcn.so')
FIELDS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
          'group_segment_fixed_size', 'max_flat_workgroup_size')
DIGEST_FIELDS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size',
                 'vgpr_spill_count', 'sgpr_spill_count')


def short_name(demangled):
    """'(anonymous namespace)::k_pwg3<2, 1, 2>(Args...)' -> 'k_pwg3<2, 1, 2>' (what rocprof's kernel trace prints)."""
    s = demangled.replace('(anonymous namespace)::', '')
    s = re.sub(r'^void ', '', s)
    depth = 0
    for i, ch in enumerate(s):
        if ch == '<':
            depth += 1
        elif ch == '>':
            depth -= 1
        elif ch == '(' and depth == 0:
            return s[:i]
    return s


def _llvm(tool, *args, **kw):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, capture_output=True, text=True, **kw).stdout


@contextlib.contextmanager
def code_objects(lib):
    """The gfx950 code objects of the library, unpacked into a temporary directory: their paths, in link order."""
    tmp = tempfile.mkdtemp(prefix='dsgcn_co_')
    try:
        local = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, local)
        _llvm('llvm-objdump', '--offloading', local, cwd=tmp)
        yield [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if 'hipv4-amdgcn' in f]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def notes(path):
    """-> {mangled kernel name: {field: int}} from one code object's metadata notes."""
    out, cur = {}, None
    for line in _llvm('llvm-readelf', '--notes', path).splitlines():
        if line.startswith('  - .'):       # a kernel's record starts at its list item: its fields are sorted, .name is not the first
            cur = {}
        m = re.match(r'\s*-?\s*\.(\w+):\s*(.*)$', line)
        if not m or cur is None:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'")
        if key == 'name' and val.startswith('_Z') and not val.endswith('.kd'):
            out[val] = cur
        elif key in FIELDS:
            cur[key] = int(val)
    return out


def symbols(path):
    """-> {symbol of .text: its disassembled instruction lines} of one code object."""
    out, sym = {}, None
    for line in _llvm('llvm-objdump', '-d', path).splitlines():
        m = re.match(r'^[0-9a-f]+ <([^>]+)>:', line)
        if m:
            sym = out.setdefault(m.group(1), [])
        elif sym is not None and line.startswith('\t'):
            sym.append(line)
    return out


def kernels(lib=DEFAULT_LIB):
    """-> {short name: {field: int}} for every kernel of every code object in the library."""
    out = {}
    with code_objects(lib) as paths:
        for path in paths:
            ks = notes(path)
            # scratch INSTRUCTIONS per kernel (the spill count of the notes also counts VGPR -> AGPR moves, which touch no
            # memory; a private segment can be reserved without a single access): what actually goes to scratch memory
            for sym, lines in symbols(path).items():
                if sym in ks:
                    ks[sym]['scratch_instructions'] = sum('scratch_' in line for line in lines)
            out.update(ks)
    names = list(out)
    dem = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True,
                         check=True).stdout.splitlines()
    return {short_name(d): out[n] for n, d in zip(names, dem)}


def digest(lib=DEFAULT_LIB):
    """One line per symbol of every code object's .text (kernels and whatever else was not inlined): code object index,
    symbol, SHA-256 of its instructions (mnemonics, operands and encodings; the address column is dropped, so a symbol
    that only moved keeps its hash), and the kernel's figures from the notes ('-' for a symbol that is no kernel).  Two
    builds generate the same code exactly when their digests are the same text: `diff` is the comparison."""
    out = []
    with code_objects(lib) as paths:
        for i, path in enumerate(paths):
            ks = notes(path)
            for sym, lines in symbols(path).items():
                # ('...' = the zero padding up to the next symbol, which the last symbol of a code object lacks: no instruction)
                text = '\n'.join(re.sub(r'// [0-9A-F]+:', '//', line) for line in lines if line.strip() != '...')
                figures = ' '.join(f"{k}={ks.get(sym, {}).get(k, '-')}" for k in DIGEST_FIELDS)
                out.append(f'{i:02d} {sym} {hashlib.sha256(text.encode()).hexdigest()} {figures}')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=DEFAULT_LIB)
    ap.add_argument('--spills', action='store_true', help='only kernels with spilled registers or a private segment')
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--digest', action='store_true', help='one line per symbol of .text: hash of its instructions + figures')
    a = ap.parse_args()
    if a.digest:
        print('\n'.join(digest(a.lib)))
        return
    ks = kernels(a.lib)
    if a.spills:
        ks = {k: v for k, v in ks.items() if v.get('vgpr_spill_count', 0) or v.get('private_segment_fixed_size', 0) or
              v.get('scratch_instructions', 0)}
    if a.json:
        json.dump(ks, sys.stdout, indent=1, sort_keys=True)
        return
    print(f'{len(ks)} kernels')
    for k in sorted(ks):
        v = ks[k]
        print(f"{v.get('vgpr_count', 0):4d} v {v.get('agpr_count', 0) or 0:4d} a  spill {v.get('vgpr_spill_count', 0):4d}  "
              f"scratch {v.get('private_segment_fixed_size', 0):5d} B / {v.get('scratch_instructions', 0):3d} instr  {k}")


if __name__ == '__main__':
    main()
