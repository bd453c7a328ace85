"""abi.py -- the ctypes signatures of the package's two libraries, read from their C headers.

The headers (include/nvbio_amd.h, include/nvbio_amd_host.h) are the one statement of the ABI: `bind` sets `restype` and `argtypes` on every
function a header declares, so that a call site passes plain Python values and a wrong count, a float for an integer or the wrong struct
raises before the library is entered.  The reader knows the C the headers are written in and no more; whatever else it meets raises.

The type rule:
    fixed-width integers, int                      their ctypes twins
    nvbio_status, nvbio_alignment_type (enums)     c_int
    const char*                                    c_char_p (as a return type too)
    an opaque handle, or a pointer to one          c_void_p
    a pointer to a struct with a registered mirror POINTER(mirror)
    every other pointer or array parameter         c_void_p (takes None, _ptr(t), byref(x) and string buffers alike)
"""
import ctypes
import os
import re

_SCALARS = {"int": ctypes.c_int, "nvbio_status": ctypes.c_int, "nvbio_alignment_type": ctypes.c_int}
_SCALARS.update({"%sint%d_t" % (u, b): getattr(ctypes, "c_%sint%d" % (u, b)) for u in ("", "u") for b in (8, 16, 32, 64)})
_HANDLES = ("nvbio_fm_index_t", "nvbio_qgram_index_t")
_DECLARATOR = re.compile(r"^((?:const\s+)?)(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w*)\s*((?:\[\s*\d+\s*\])?)$")


class Header:
    """prototypes : name -> (return type, [(C type, parameter name)]), the C type spelled without spaces ("const nvbio_string_set*")
    structs    : name -> [(field name, ctypes type)], in declaration order
    known      : the struct names a pointer may point to: this header's and those of the headers it includes with quotes"""

    def __init__(self, path):
        raw = open(path).read()
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", raw, flags=re.S)
        text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)                       # preprocessor lines, continued ones whole
        text = re.sub(r'extern\s+"C"\s*\{', " ", text)
        text = re.sub(r"(?:typedef\s+)?enum\s*\{[^{}]*\}\s*\w*\s*;", " ", text)
        text = re.sub(r"typedef\s+struct\s+\w+\s*\*\s*\w+\s*;", " ", text)                           # the opaque handles (_HANDLES)
        self.structs, self.known = {}, set()
        for inc in re.findall(r'^[ \t]*#\s*include\s+"([^"]+)"', raw, flags=re.M):
            self.known |= Header(os.path.join(os.path.dirname(path), inc)).known
        bodies = re.findall(r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", text)
        self.known |= {name for _, name in bodies}
        for body, name in bodies:
            self.structs[name] = [f for line in body.split(";") if line.strip() for f in self._fields(line, name)]
        text = re.sub(r"typedef\s+struct\s*\{[^{}]*\}\s*\w+\s*;", " ", text)
        self.prototypes = {}
        for stmt in text.replace("}", " ").split(";"):                                               # what is left: prototypes, and extern "C"'s brace
            if not stmt.strip():
                continue
            m = re.match(r"^\s*(.*?)\b(nvbio_\w+)\s*\((.*)\)\s*$", stmt, flags=re.S)
            if not m or m.group(2) in self.prototypes:
                raise ValueError("%s: cannot read `%s` as a prototype" % (path, " ".join(stmt.split())))
            params = [] if m.group(3).strip() in ("", "void") else [self._declarator(p, m.group(2)) for p in m.group(3).split(",")]
            self.prototypes[m.group(2)] = (self._declarator(m.group(1), m.group(2))[0], [(t + "*" if dim else t, n) for t, n, dim in params])

    def _declarator(self, decl, where):
        """`const uint32_t* rows_dev` -> ("const uint32_t*", "rows_dev", ""); an array's `[n]` comes third"""
        m = _DECLARATOR.match(" ".join(decl.split()))
        if not m:
            raise ValueError("%s: cannot read the declarator `%s`" % (where, decl.strip()))
        const, base, stars, name, dim = m.groups()
        if base not in _SCALARS and base not in _HANDLES and base not in self.known and base not in ("void", "char"):
            raise ValueError("%s: unknown type `%s`" % (where, base))
        return ("const " if const else "") + base + "*" * stars.count("*"), name, dim.strip("[] ")

    def _fields(self, line, where):
        """one member declaration, `const uint32_t* a_dev` or `uint32_t x, y, L2[5]` -> [(name, ctypes type)]"""
        first, *rest = line.split(",")
        ctype, name, dim = self._declarator(first, where)
        base = ctype.rstrip("*")
        out = []
        for ctype, name, dim in [(ctype, name, dim)] + [self._declarator(base + " " + r, where) for r in rest]:
            t = self.ctype(ctype, {})
            out.append((name, t * int(dim) if dim else t))
        return out

    def ctype(self, ctype, mirrors):
        """the type rule of this module's header comment; mirrors: C struct name -> ctypes.Structure"""
        base = ctype.replace("const ", "").rstrip("*")
        depth = len(ctype) - len(ctype.rstrip("*"))
        if depth == 0:
            if base == "void":
                return None
            if base in _SCALARS or base in _HANDLES:
                return _SCALARS.get(base, ctypes.c_void_p)
            raise ValueError("`%s` by value has no ctypes type" % ctype)
        if ctype == "const char*":
            return ctypes.c_char_p
        return ctypes.POINTER(mirrors[base]) if depth == 1 and base in mirrors else ctypes.c_void_p


def bind(cdll, header_path, mirrors):
    """set restype and argtypes on every function of `cdll` that the header declares; a declared function the library does not export raises"""
    header = Header(header_path)
    for name, (ret, params) in header.prototypes.items():
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            raise AttributeError("%s declares %s, which %s does not export" % (header_path, name, cdll._name)) from None
        fn.restype = header.ctype(ret, mirrors)
        fn.argtypes = [header.ctype(t, mirrors) for t, _ in params]
