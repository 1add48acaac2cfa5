"""Loader/builder for ``libdsgcn.so`` — the C-ABI HIP library (declared in ``include/dsgcn.h``).

The library is built in-tree (``ds-gcn_amd/lib/libdsgcn.so``) with ``hipcc --offload-arch=gfx950`` and
loaded with ``ctypes``: no torch types cross the boundary, only raw device pointers, sizes and the
HIP stream handle.  The binding itself (argtypes, result types, job records) is read from the headers by ``cheader``:
nothing of the ABI is typed here.  ``lib()`` raises if the library is missing — there is no fallback.
"""
import ctypes
import glob
import os
import subprocess

from . import cheader

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_DIR = os.path.join(_HERE, 'lib')
LIB_PATH = os.path.join(LIB_DIR, 'libdsgcn.so')
LAB_LIB_PATH = os.path.join(LIB_DIR, 'libdsgcn_lab.so')
INCLUDE = os.path.join(os.path.dirname(_HERE), 'include')

_lib = None
_lab = None
# matmul precision level the library starts at (kernels.py sets it from DSGCN_MATMUL_PRECISION before the first load)
INITIAL_MATMUL_PRECISION = 0


def _header(name, structs=()):
    with open(os.path.join(INCLUDE, name)) as f:
        return cheader.read(f.read(), structs, where='include/' + name)


# The binding is what the headers declare: each definition in csrc/ is compiled against the same prototypes (common.h
# includes them), and cheader raises here, at import, on any C it cannot read.
_jobs = _header('dsgcn_jobs.h')
_abi = _header('dsgcn.h', _jobs.structs)
_lab_abi = _header('dsgcn_lab.h', _jobs.structs)        # measurement-only entry points: exported by libdsgcn_lab.so only

# name -> argtypes (any pointer: c_void_p); every entry point returns int (0 ok, >0 hipError_t, <0 argument error) ...
SIGNATURES = {name: args for name, (_, args) in _abi.functions.items()}
LAB_SIGNATURES = {name: args for name, (_, args) in _lab_abi.functions.items()}
# ... except the few the header gives a size_t
SIZE_T_RESULTS = {name for name, (res, _) in {**_abi.functions, **_lab_abi.functions}.items() if res is ctypes.c_size_t}

# The job records of include/dsgcn_jobs.h as ctypes.Structure classes, named after their typedefs (dsgcn_bn_fin_job ->
# BnFinJob): BnFinJob, BnCoefJob, Dropout, CtrPrepJob, CtrFinJob, TsplitJob, GuestConv (its field `in` is `inp` here).
globals().update({cheader.class_name(typedef): cls for typedef, cls in _jobs.structs.items()})
BN_JOBS_MAX = _jobs.defines['DSGCN_BN_JOBS_MAX']


def sources(lab=False):
    """Product sources; lab=True adds csrc/lab/*.hip (measurement-only kernels: never part of libdsgcn.so)."""
    srcs = sorted(glob.glob(os.path.join(CSRC, '*.hip')))
    if lab:
        srcs += sorted(glob.glob(os.path.join(CSRC, 'lab', '*.hip')))
    return srcs


def _source_hash(lab=False):
    import hashlib
    h = hashlib.sha256()
    extra = sorted(glob.glob(os.path.join(CSRC, 'lab', '*.h'))) if lab else []
    for path in (sources(lab) + sorted(glob.glob(os.path.join(CSRC, '*.h'))) + extra +
                 sorted(glob.glob(os.path.join(INCLUDE, '*.h')))):
        with open(path, 'rb') as f:
            h.update(os.path.basename(path).encode())
            h.update(f.read())
    return h.hexdigest()


def _file_hash(paths):
    import hashlib
    h = hashlib.sha256()
    for path in paths:
        with open(path, 'rb') as f:
            h.update(os.path.basename(path).encode())
            h.update(f.read())
    return h.hexdigest()


def build(force=False, verbose=False, lab=False):
    """Compile every HIP source for gfx950 into one shared library (cross-compiles without a GPU).
    lab=True builds ``libdsgcn_lab.so`` instead: the same sources with -DDSGCN_LAB, which adds the measurement-only
    entry points of include/dsgcn_lab.h (used by tools/, never by the package).
    Up-to-date check = content hash of the sources (file times do not survive the copy to a GPU box).  Each source is
    compiled to its own object (cached under lib/obj by content hash of the source + headers, compiled in parallel),
    then linked."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = sources(lab)
    lib_path = LAB_LIB_PATH if lab else LIB_PATH
    stamp = lib_path + '.srchash'
    digest = _source_hash(lab)
    if not force and os.path.exists(lib_path) and os.path.exists(stamp):
        with open(stamp) as f:
            if f.read().strip() == digest:
                return lib_path
    obj_dir = os.path.join(LIB_DIR, 'obj_lab' if lab else 'obj')
    os.makedirs(obj_dir, exist_ok=True)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    headers = sorted(glob.glob(os.path.join(CSRC, '*.h'))) + sorted(glob.glob(os.path.join(INCLUDE, '*.h')))
    if lab:
        headers += sorted(glob.glob(os.path.join(CSRC, 'lab', '*.h')))
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-I', INCLUDE, '-I', CSRC]
    if lab:
        flags.append('-DDSGCN_LAB')
        flags += [f for f in os.environ.get('DSGCN_LAB_FLAGS', '').split() if f]      # e.g. -DKA_NT_LOADS=1 for an A/B build
    jobs, objs = [], []
    for src in srcs:
        base = os.path.splitext(os.path.basename(src))[0]
        obj = os.path.join(obj_dir, f'{base}.{_file_hash([src] + headers)[:16]}.o')
        objs.append(obj)
        if force or not os.path.exists(obj):
            for old in glob.glob(os.path.join(obj_dir, base + '.*.o')):
                os.remove(old)
            jobs.append([hipcc] + flags + ['-c', src, '-o', obj])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(run, jobs))
    run([hipcc, '--offload-arch=gfx950', '-fPIC', '-shared', '-o', lib_path] + objs)
    with open(stamp, 'w') as f:
        f.write(digest)
    return lib_path


def _bind(handle, signatures, missing_ok=False):
    for name, argtypes in signatures.items():
        if missing_ok and not hasattr(handle, name):
            continue
        fn = getattr(handle, name)      # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = ctypes.c_size_t if name in SIZE_T_RESULTS else ctypes.c_int
    return handle


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'dsgcn: {LIB_PATH} is missing — build it with `python -c "import __graft_entry__ as g; g.build()"`. '
                'The HIP library is the only implementation of the hot path (no CPU/eager fallback).')
        handle = _bind(ctypes.CDLL(LIB_PATH), SIGNATURES)
        if INITIAL_MATMUL_PRECISION:
            check(handle.dsgcn_set_matmul_precision(INITIAL_MATMUL_PRECISION), 'dsgcn_set_matmul_precision')
        _lib = handle
    return _lib


def lab_lib():
    """``libdsgcn_lab.so`` (product + measurement-only entry points), built on first use.  tools/ only."""
    global _lab
    if _lab is None:
        # DSGCN_LAB_LIB: an A/B run of tools/ against another build of the lab library (e.g. the previous round's kernels)
        other = os.environ.get('DSGCN_LAB_LIB')
        # (an older build under A/B: entry points added since are simply absent)
        handle = _bind(ctypes.CDLL(other or build(lab=True)), {**SIGNATURES, **LAB_SIGNATURES}, missing_ok=bool(other))
        _lab = handle
    return _lab


class DsgcnError(RuntimeError):
    pass


def check(code, what):
    if code != 0:
        kind = 'argument rejected' if code < 0 else 'hipError_t'
        raise DsgcnError(f'{what} failed: {kind} {code}')


_dynadj_range = {}


def dynadj_require_backward(mid, V, E, ld=32, who='dynadj'):
    """K-B's forward holds shapes its backward does not (the backward keeps P_e / Q_e of all ``mid`` channels plus its
    gradient scratch in LDS; ``dsgcn_dynadj_supported`` is the one statement of both ranges).  Raises NotImplementedError
    where a backward of this shape could not launch — asked before the forward runs, by whoever is about to record one."""
    key = (mid, V, E, ld)
    if key not in _dynadj_range:
        ok = lib().dsgcn_dynadj_supported
        msg = None
        if ok(1, mid, V, ld, E, 1) != 0:
            top = max([m for m in range(1, 65) if ok(1, m, V, ld, E, 1) == 0], default=0)
            if top:                     # (no mid fits: V, E or ld is out of range, and the forward's launch says so)
                msg = (f'mid = {mid} at V = {V} joints, E = {E} edge classes: the K-B backward holds mid <= {top} at '
                       'this V and E (its LDS image), so this shape evaluates under torch.no_grad() but cannot train')
        _dynadj_range[key] = msg
    if _dynadj_range[key] is not None:
        raise NotImplementedError(f'{who}: {_dynadj_range[key]}')
