"""CPU-only: the C-ABI library loads and exports every symbol include/nvbio_amd.h declares;
compute entry points fail loudly (no CPU fallback) when there is no GPU.  The ctypes side is held to the two headers: every declared
function is bound with its signature, every struct mirror equals its header struct, every call site in the package passes the
declared number of arguments, and misuse raises before a library is entered."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge


def _declared(path=None):
    amd = ge.load_package()
    txt = open(path or amd.HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nvbio_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported():
    amd = ge.load_package()
    # through lib(), which loads torch's HIP runtime first: a bare CDLL as the first load binds the library to another runtime
    # for the rest of the process, and on a GPU every later test in it then sees NVBIO_ERR_NO_DEVICE
    L = amd.lib()
    names = _declared()
    assert len(names) >= 18
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_version_and_error_string():
    amd = ge.load_package()
    assert amd.lib().nvbio_amd_version() == 100
    assert isinstance(amd.lib().nvbio_amd_last_error(), bytes)


def test_no_cpu_fallback():
    """without a GPU every compute call must raise, never silently compute on the host"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    amd = ge.load_package()
    v = amd._View()
    v.length, v.primary = 64, 1
    for i, x in enumerate((0, 16, 32, 48, 64)):
        v.L2[i] = x
    buf = np.zeros(64, dtype=np.uint32)
    addr = buf.ctypes.data
    addr += (32 - addr % 32) % 32
    v.bwt_occ_dev, v.bwt_occ_words = addr, 8
    h = ctypes.c_void_p()
    st = amd.lib().nvbio_fm_index_create(ctypes.byref(v), 0, 0, None, ctypes.byref(h))
    assert st == 5, st                                  # NVBIO_ERR_NO_DEVICE
    assert b"no CPU fallback" in amd.lib().nvbio_amd_last_error() or b"device" in amd.lib().nvbio_amd_last_error()


def test_product_does_not_import_the_oracle():
    import os
    amd = ge.load_package()
    pkg = os.path.dirname(amd.__file__)
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(root, f)).read()
                assert "import oracle" not in src and "liboracle" not in src and "nvbio_oracle" not in src, f


# ---- the ctypes side against the two headers ---------------------------------------------------------------------------------------
_INTS = {"int": ctypes.c_int, "nvbio_status": ctypes.c_int, "nvbio_alignment_type": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32,
         "uint64_t": ctypes.c_uint64}
# structs of either header that deliberately have no Python mirror: elements of device arrays, which Python never builds or reads one by one
UNMIRRORED = {"nvbio_uint2", "nvbio_mem_range", "nvbio_mem_hit"}
# the host-loop calls of pipeline.py, whose arguments are put together from the tuples head, kind and tail
STARRED = {"nvbio_host_best_approx", "nvbio_host_best_approx_ragged", "nvbio_host_best_approx_paired", "nvbio_host_best_approx_paired_ragged"}


def _bound():
    """[(library, header path, parsed header)] of the package's two libraries, and its registry of mirrors"""
    amd = ge.load_package()
    from importlib import import_module
    pipeline = import_module("nvbio_gpl_amd.pipeline")
    return [(L, path, amd.abi.Header(path)) for L, path in ((amd.lib(), amd.HEADER_PATH), (pipeline._host_lib(), amd.HOST_HEADER_PATH))], pipeline._HOST_MIRRORS


def test_every_declared_function_is_bound_with_its_signature():
    libs, mirrors = _bound()
    counts = []
    for L, path, header in libs:
        assert sorted(header.prototypes) == _declared(path)              # the loose scan: a prototype the reader cannot parse is a failure, not a gap
        for name, (ret, params) in header.prototypes.items():
            fn = getattr(L, name)
            assert fn.restype is {"void": None, "const char*": ctypes.c_char_p}.get(ret, ctypes.c_int), (name, ret)
            assert ret in ("void", "const char*", "int", "nvbio_status"), (name, ret)
            assert len(fn.argtypes) == len(params), name
            for (ctype, pname), bound in zip(params, fn.argtypes):
                base = ctype.replace("const ", "").rstrip("*")
                if not ctype.endswith("*"):
                    want = _INTS.get(ctype, ctypes.c_void_p)             # what is no integer is an opaque handle
                    assert ctype in _INTS or ctype.endswith("_t"), (name, pname, ctype)
                elif ctype == "const char*":
                    want = ctypes.c_char_p
                elif base in mirrors and not ctype.endswith("**"):
                    want = ctypes.POINTER(mirrors[base])
                else:
                    want = ctypes.c_void_p
                assert bound is want, (name, pname, ctype, bound)
        counts.append(len(header.prototypes))
    assert counts[0] >= 156 and counts[1] == 7, counts


def _natural_size(fields):
    """sizeof a C struct of these (name, ctypes type) members under natural alignment"""
    offset = biggest = 0
    for _, t in fields:
        align = ctypes.sizeof(getattr(t, "_type_", t) if hasattr(t, "_length_") else t)
        offset = (offset + align - 1) // align * align + ctypes.sizeof(t)
        biggest = max(biggest, align)
    return (offset + biggest - 1) // biggest * biggest


def test_every_mirror_equals_its_header_struct():
    libs, mirrors = _bound()
    structs = {}
    for _, _, header in libs:
        assert not set(header.structs) & set(structs)
        structs.update(header.structs)
    assert set(structs) - set(mirrors) == UNMIRRORED                      # a new struct needs a mirror and a line in the registry, or a line here
    assert not set(mirrors) - set(structs)
    shape = lambda t: (t._type_, t._length_) if hasattr(t, "_length_") else t
    for name, mirror in mirrors.items():
        assert [(f, shape(t)) for f, t in mirror._fields_] == [(f, shape(t)) for f, t in structs[name]], name
        assert ctypes.sizeof(mirror) == _natural_size(structs[name]), name
    assert ctypes.sizeof(mirrors["nvbio_alignment_batch"]) == 104 and ctypes.sizeof(mirrors["nvbio_fm_index_view"]) == 72          # counted by hand


def test_every_call_site_passes_the_declared_number_of_arguments():
    """static, so that it reaches the call paths that only run on a GPU: ctypes itself only catches too few arguments"""
    libs, _ = _bound()
    amd = ge.load_package()
    prototypes = {}
    for _, _, header in libs:
        prototypes.update(header.prototypes)
    seen, starred = 0, set()
    for fname in ("__init__.py", "pipeline.py"):
        tree = ast.parse(open(os.path.join(os.path.dirname(amd.__file__), fname)).read())
        for func in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.Module))]:
            # the tuples a function (or the module) assigns to one name once: what a starred argument of a call in it unpacks
            tuples = {}
            for n in ast.walk(func):
                if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name):
                    tuples.setdefault(n.targets[0].id, []).append(n.value)
            for call in [n for n in ast.walk(func) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr.startswith("nvbio_")]:
                if isinstance(func, ast.Module) and any(call in ast.walk(f) for f in ast.walk(tree) if isinstance(f, ast.FunctionDef)):
                    continue                                              # counted with its function
                name, n_args = call.func.attr, 0
                assert name in prototypes and not call.keywords, (fname, call.lineno, name)
                for a in call.args:
                    if isinstance(a, ast.Starred):
                        starred.add(name)
                        values = tuples.get(a.value.id, [])
                        assert len(values) == 1 and isinstance(values[0], ast.Tuple), (fname, call.lineno, a.value.id)
                        n_args += len(values[0].elts)
                    else:
                        n_args += 1
                assert n_args == len(prototypes[name][1]), (fname, call.lineno, name, n_args)
                seen += 1
    assert starred == STARRED and seen >= 120, (starred, seen)


def test_misuse_raises_before_the_library_is_entered():
    amd = ge.load_package()
    L = amd.lib()
    nb = ctypes.c_uint64(0)
    wrong = (TypeError, ctypes.ArgumentError)
    with pytest.raises(wrong):
        L.nvbio_fm_rank4(None, None, 4)                                   # too few arguments
    with pytest.raises(wrong):
        L.nvbio_text_planes_bytes(1.5, ctypes.byref(nb))                  # a float for a uint32_t
    with pytest.raises(wrong):
        L.nvbio_banded_gotoh_traceback_temp_bytes(ctypes.byref(amd._StringSet()), 31, ctypes.byref(nb))      # a nvbio_alignment_batch* is declared
    assert L.nvbio_text_planes_bytes(1000, ctypes.byref(nb)) == 0 and nb.value > 0
