"""CPU: the C ABI has one statement.  ``cheader`` reads the forms the headers use and refuses the rest; the job records it
builds have the compiler's sizes and offsets; every source reaches ``include/dsgcn.h`` through its includes, so each
definition is compiled against its prototype; one host-only entry point with out-parameters runs through the binding."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

from dsgcn_amd import cheader, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')
CSRC = os.path.join(ROOT, 'ds-gcn_amd', 'csrc')

I, F, D, L, LL, P = (ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_long, ctypes.c_longlong, ctypes.c_void_p)

SYNTHETIC = '''
/* a comment with (parentheses); semicolons; and a prototype-shaped int dsgcn_ghost(int x); inside */
#ifndef X_H
#define X_H
#include <stddef.h>
#define DSGCN_X_JOBS_MAX 12
#define DSGCN_EINVAL (-1)
#ifdef __cplusplus
extern "C" {
#endif
typedef struct {
  const float* a; float* b;       /* two declarations on a line; (see) */
  double count;                   // a line comment; with (both)
  float eps;
  int K, Co, R, reserved;
  long n; long long m;
  unsigned int call; unsigned long long seed;
  const long long* step;
  void* ws;
  const float* w[4];
  float* in;
} dsgcn_x_job;

int dsgcn_none(void);
size_t dsgcn_bytes(int a, float b, double c, long d, long long e);
int dsgcn_pointers(const float* x, float* y, const int* idx, const float* const* table, void** out,
                   const dsgcn_x_job* jobs, int* hosted,
                   void* stream);   /* spans three lines */
#ifdef __cplusplus
}
#endif
#endif
'''


def test_reader_takes_every_form_the_headers_use():
    h = cheader.read(SYNTHETIC, where='x.h')
    assert h.functions == {'dsgcn_none': (I, []),
                           'dsgcn_bytes': (ctypes.c_size_t, [I, F, D, L, LL]),
                           'dsgcn_pointers': (I, [P] * 8)}
    assert list(h.functions) == ['dsgcn_none', 'dsgcn_bytes', 'dsgcn_pointers']
    assert h.defines == {'DSGCN_X_JOBS_MAX': 12}
    assert list(h.structs) == ['dsgcn_x_job']
    job = h.structs['dsgcn_x_job']
    assert job.__name__ == 'XJob' and issubclass(job, ctypes.Structure)
    assert job._fields_ == [('a', P), ('b', P), ('count', D), ('eps', F), ('K', I), ('Co', I), ('R', I), ('reserved', I),
                            ('n', L), ('m', LL), ('call', ctypes.c_uint), ('seed', ctypes.c_ulonglong), ('step', P),
                            ('ws', P), ('w', P * 4), ('inp', P)]
    assert cheader.class_name('dsgcn_bn_fin_job') == 'BnFinJob' and cheader.class_name('dsgcn_dropout') == 'Dropout'
    # a record of a header read before may stand behind a pointer; one nobody declared may not
    assert cheader.read('int dsgcn_f(const dsgcn_x_job* j);', structs=h.structs).functions == {'dsgcn_f': (I, [P])}
    with pytest.raises(cheader.HeaderError):
        cheader.read('int dsgcn_f(const dsgcn_x_job* j);')


REFUSED = {
    'unknown type word': 'int dsgcn_f(short x);',
    'unknown pointer type': 'int dsgcn_f(const half* x);',
    'unsigned is for records only': 'int dsgcn_f(unsigned int x);',
    'parameter without a name': 'int dsgcn_f(int, float b);',
    'pointer parameter without a name': 'int dsgcn_f(const float*);',
    'function pointer': 'int dsgcn_f(int (*cb)(int), int n);',
    'variadic': 'int dsgcn_f(int n, ...);',
    'star on the declarator': 'int dsgcn_f(float *x);',
    'array parameter': 'int dsgcn_f(int x[4]);',
    'empty parameter list': 'int dsgcn_f();',
    'unknown result': 'float dsgcn_f(int x);',
    'not a dsgcn_ name': 'int other_f(int x);',
    'declared twice': 'int dsgcn_f(int x);\nint dsgcn_f(int x);',
    'a body': 'int dsgcn_f(int x) { return x; }',
    'bit field': 'typedef struct { int a : 3; } dsgcn_t;',
    'nested struct': 'typedef struct { struct { int a; } in; int b; } dsgcn_t;',
    'star on a field declarator': 'typedef struct { float *a; } dsgcn_t;',
    'two declarators after a pointer': 'typedef struct { float* a, b; } dsgcn_t;',
    'unknown field type': 'typedef struct { char c; } dsgcn_t;',
    'keyword field without an entry': 'typedef struct { int class; } dsgcn_t;',
    'continued preprocessor line': '#define DSGCN_F(x) \\\n  (x)\nint dsgcn_f(int x);',
}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_reader_refuses(what):
    with pytest.raises(cheader.HeaderError):
        cheader.read(REFUSED[what])


def test_refusal_names_the_header_line():
    text = SYNTHETIC.replace('int dsgcn_none(void);', 'int dsgcn_none(void);\nint dsgcn_new(__half x);')
    line = text[:text.index('dsgcn_new')].count('\n') + 1
    with pytest.raises(cheader.HeaderError, match=rf'^x\.h:{line}: .*__half'):
        cheader.read(text, where='x.h')
    # no prototype-shaped text of the real headers is left unread: what the reader yields is every `dsgcn_name(` outside
    # comments (test_native_abi.py counts the same with its own expression)
    for name, table in (('dsgcn.h', native.SIGNATURES), ('dsgcn_lab.h', native.LAB_SIGNATURES)):
        with open(os.path.join(INCLUDE, name)) as f:
            code = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
        assert re.findall(r'\b(dsgcn_\w+)\s*\(', code) == list(table)


RECORDS = ('BnFinJob', 'BnCoefJob', 'Dropout', 'CtrPrepJob', 'CtrFinJob', 'TsplitJob', 'GuestConv')


def test_job_records_match_the_compiler(tmp_path):
    structs, defines = native._jobs.structs, native._jobs.defines
    assert tuple(cheader.class_name(t) for t in structs) == RECORDS
    assert all(getattr(native, cheader.class_name(t)) is cls for t, cls in structs.items())
    c_names = {v: k for k, v in cheader.RENAMED_FIELDS.items()}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsgcn_jobs.h"', 'int main(void) {']
    for typedef, cls in structs.items():
        lines.append(f'  printf("{typedef} %zu", sizeof({typedef}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf(" {field}@%zu", offsetof({typedef}, {c_names.get(field, field)}));')
        lines.append('  printf("\\n");')
    lines += [f'  printf("{d} %d\\n", {d});' for d in defines]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'records.c', tmp_path / 'records'
    src.write_text('\n'.join(lines) + '\n')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '-x', 'c', str(src), '-I', INCLUDE, '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    ours = [f'{typedef} {ctypes.sizeof(cls)}' + ''.join(f' {f}@{getattr(cls, f).offset}' for f, _ in cls._fields_)
            for typedef, cls in structs.items()]
    ours += [f'{d} {v}' for d, v in defines.items()]
    assert out == ours
    assert len(structs) == 7 and sum(len(cls._fields_) for cls in structs.values()) >= 50
    assert set(defines) == {'DSGCN_BN_JOBS_MAX', 'DSGCN_CTR_JOBS_MAX', 'DSGCN_TSPLIT_JOBS_MAX'}
    assert native.BN_JOBS_MAX == defines['DSGCN_BN_JOBS_MAX']


def _includes(path):
    """[(quoted include resolved under csrc/ or include/, it stands under `#ifdef DSGCN_LAB`)] of one file."""
    out, guards = [], []
    with open(path) as f:
        for line in f:
            m = re.match(r'\s*#\s*(ifdef|ifndef|if|else|elif|endif|include)\b\s*(.*)', line)
            if not m:
                continue
            word, rest = m.groups()
            if word in ('ifdef', 'ifndef', 'if'):
                guards.append(word == 'ifdef' and rest.split()[0] == 'DSGCN_LAB')
            elif word in ('else', 'elif'):
                guards[-1] = False
            elif word == 'endif':
                guards.pop()
            elif rest.startswith('"'):
                name = rest.split('"')[1]
                for base in (os.path.dirname(path), CSRC, INCLUDE):
                    if os.path.exists(os.path.join(base, name)):
                        out.append((os.path.normpath(os.path.join(base, name)), any(guards)))
                        break
                else:
                    raise AssertionError(f'{path}: cannot find "{name}"')
    return out


def _reached(path, lab, seen=None):
    """Headers reached from path through quoted includes; lab=False: as compiled without -DDSGCN_LAB."""
    seen = set() if seen is None else seen
    for header, guarded in _includes(path):
        if header not in seen and (lab or not guarded):
            seen.add(header)
            _reached(header, lab, seen)
    return seen


def test_every_source_is_compiled_against_the_header():
    sources = sorted(glob.glob(os.path.join(CSRC, '*.hip'))) + sorted(glob.glob(os.path.join(CSRC, 'lab', '*.hip')))
    assert len(sources) >= 32 and sources == native.sources(lab=True)
    product, lab = os.path.join(INCLUDE, 'dsgcn.h'), os.path.join(INCLUDE, 'dsgcn_lab.h')
    for src in sources:
        assert product in _reached(src, lab=False), f'{src} does not reach include/dsgcn.h'
        assert lab not in _reached(src, lab=False), f'{src} reaches include/dsgcn_lab.h outside #ifdef DSGCN_LAB'
        assert lab in _reached(src, lab=True), f'{src} does not reach include/dsgcn_lab.h under -DDSGCN_LAB'
    # the error codes (and so every other #define of the ABI) have one copy
    defining = [p for p in glob.glob(os.path.join(ROOT, 'include', '*.h')) + glob.glob(os.path.join(CSRC, '**', '*.*'),
                                                                                         recursive=True)
                if re.search(r'#\s*define\s+DSGCN_E(INVAL|UNSUPPORTED)\b', open(p).read())]
    assert defining == [product]


def test_pwconv_plan_through_the_binding():
    # a pure host query with three int* out-parameters: one of the rows whose pointers are now c_void_p
    assert native.SIGNATURES['dsgcn_pwconv_plan'] == [I, I, I, P, P, P]
    a, b, c = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert native.lib().dsgcn_pwconv_plan(64, 25, 1, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    assert a.value > 0 and b.value > 0 and c.value > 0
