"""Reads the C ABI out of ``include/*.h`` so that ``native`` binds what the headers declare and nothing is typed twice.

Pure Python: imports neither torch nor the library.  It reads the subset of C these headers are written in (prototypes
``int|size_t dsgcn_name(params);``, ``typedef struct { ... } dsgcn_x;`` records of scalars, pointers and pointer arrays,
``#define DSGCN_*_MAX n``) and raises ``HeaderError`` with the line number on anything else, so that a new form in a
header is a CPU failure at import and never a mis-bound call."""
import ctypes
import keyword
import re

SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'long': ctypes.c_long,
           'long long': ctypes.c_longlong}
FIELD_SCALARS = {**SCALARS, 'unsigned int': ctypes.c_uint, 'unsigned long long': ctypes.c_ulonglong}
RESULTS = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t}
RENAMED_FIELDS = {'in': 'inp'}      # C field names that are Python keywords (dsgcn_guest_conv.in)

_TYPE_WORDS = {w for t in FIELD_SCALARS for w in t.split()} | {'const', 'void'}
_ITEM = re.compile(r'''(?P<wrap>extern\s+"C"\s*\{|\})
                     | typedef\s+struct\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;
                     | (?P<ret>\w+)\s+(?P<fn>\w+)\s*\((?P<params>[^();{}]*)\)\s*;''', re.X)


class HeaderError(ValueError):
    pass


class Header:
    """functions: name -> (restype, [argtype...]);  structs: typedef name -> ctypes.Structure;  defines: name -> int."""

    def __init__(self):
        self.functions, self.structs, self.defines = {}, {}, {}


def class_name(typedef):
    """dsgcn_bn_fin_job -> BnFinJob"""
    return ''.join(w.capitalize() for w in typedef.split('_')[1:])


def _declare(decl, scalars, structs, fail):
    """One declaration ('const float* const* x', 'int K, Co', 'float* out[4]') -> [(name, ctype), ...]."""
    if re.search(r'\*\w', decl):
        fail(f"'*' attached to the declarator in '{decl}': write 'T* name'")
    tok = re.findall(r'\w+|\.\.\.|\S', decl)
    if not tok:
        fail('an empty declaration')
    if '*' in tok:
        first, end = tok.index('*'), len(tok) - tok[::-1].index('*')
        if set(tok[first:end]) - {'*', 'const'}:
            fail(f"cannot read '{decl}'")
        base, ctype = ' '.join(t for t in tok[:first] if t != 'const'), ctypes.c_void_p
        if base not in FIELD_SCALARS and base != 'void' and base not in structs:
            fail(f"unknown type '{base}' in '{decl}'")
        if tok[end:end + 1] == ['const']:       # 'T* const name'
            end += 1
    else:
        end = next((i for i, t in enumerate(tok) if t not in _TYPE_WORDS), len(tok))
        base = ' '.join(t for t in tok[:end] if t != 'const')
        if base not in scalars:
            fail(f"unknown type '{base or tok[0]}' in '{decl}'")
        ctype = scalars[base]
    out = []
    for d in ''.join(tok[end:]).split(','):
        m = re.fullmatch(r'([A-Za-z_]\w*)(?:\[(\d+)\])?', d)
        if not m or m.group(1) in _TYPE_WORDS:
            fail(f"no name, or a form this reader does not take (bit field, function pointer, '...'), in '{decl}'")
        out.append((m.group(1), ctype * int(m.group(2)) if m.group(2) else ctype))
    if len(out) > 1 and ctype is ctypes.c_void_p:
        fail(f"several declarators after a pointer type in '{decl}': one per declaration")
    return out


def read(text, structs=(), where='header'):
    """Parse one header's text.  structs: typedef names (of a header read before) that may appear behind a pointer."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', lambda m: '\n' * m.group().count('\n'), text, flags=re.S)
    h = Header()
    known = set(structs)
    lines = text.split('\n')
    for i, line in enumerate(lines):
        if line.lstrip().startswith('#'):
            if line.rstrip().endswith('\\'):
                raise HeaderError(f'{where}:{i + 1}: a continued preprocessor line')
            m = re.fullmatch(r'\s*#\s*define\s+(DSGCN_\w+_MAX)\s+(\d+)\s*', line)
            if m:
                h.defines[m.group(1)] = int(m.group(2))
            lines[i] = ''
    text = '\n'.join(lines)
    pos = 0
    while True:
        pos = re.compile(r'\s*').match(text, pos).end()
        if pos == len(text):
            return h
        lineno = text.count('\n', 0, pos) + 1

        def fail(msg):
            raise HeaderError(f'{where}:{lineno}: {msg}')

        m = _ITEM.match(text, pos)
        if not m:
            fail(f"cannot read '{text[pos:].split(chr(10), 1)[0].strip()}'")
        pos = m.end()
        if m.group('struct'):
            fields = []
            for decl in m.group('body').split(';'):
                if decl.strip():
                    fields += _declare(decl.strip(), FIELD_SCALARS, known, fail)
            for name, _ in fields:
                if keyword.iskeyword(name) and name not in RENAMED_FIELDS:
                    fail(f"field '{name}' is a Python keyword: give it an entry in RENAMED_FIELDS")
            typedef = m.group('struct')
            h.structs[typedef] = type(class_name(typedef), (ctypes.Structure,), {
                '__doc__': f'{where}: {typedef}', '_fields_': [(RENAMED_FIELDS.get(n, n), t) for n, t in fields]})
            known.add(typedef)
        elif m.group('fn'):
            ret, name, params = m.group('ret'), m.group('fn'), m.group('params').strip()
            if ret not in RESULTS or not name.startswith('dsgcn_'):
                fail(f"an entry point is 'int|size_t dsgcn_name(...)', not '{ret} {name}'")
            args = []
            if params != 'void':
                for p in params.split(','):
                    (_, ctype), = _declare(p.strip(), SCALARS, known, fail)
                    if issubclass(ctype, ctypes.Array):
                        fail(f"array parameter '{p.strip()}'")
                    args.append(ctype)
            if name in h.functions:
                fail(f'{name} is declared twice')
            h.functions[name] = (RESULTS[ret], args)
