"""The one reader of include/mvx_hip.h for the host tests: every declaration of the C ABI as ctypes types, to be held against
``Extension.PROTOTYPES`` and to build argument lists by parameter name."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mvx_hip.h')
CTYPES = {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32,
          'uint64_t': ctypes.c_uint64, 'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double, 'void': None}
_DECLARATIONS = None


def _ctype(decl):
    """ctypes type of ``[const] type [*]`` (a parameter with its name cut off, or a result): any pointer is c_void_p."""
    return ctypes.c_void_p if '*' in decl else CTYPES[decl.replace('const ', '').strip()]


def declarations():
    """{name: (result ctype, [(parameter name, ctype)])} of every ``mvx_*`` function the header declares (read once)."""
    global _DECLARATIONS
    if _DECLARATIONS is None:
        text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
        _DECLARATIONS = {}
        for result, name, params in re.findall(r'([\w \*]+?)\b(mvx_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;', text, flags=re.S):
            assert name not in _DECLARATIONS, name
            out = []
            for q in (' '.join(p.split()) for p in params.split(',')):
                if q not in ('', 'void'):
                    pname = re.search(r'(\w+)$', q).group(1)
                    out.append((pname, _ctype(q[:-len(pname)])))
            _DECLARATIONS[name] = (_ctype(' '.join(result.split())), out)
    return _DECLARATIONS


def parameter_names(name):
    return [p for p, _ in declarations()[name][1]]


def parameter_types(name):
    return [t for _, t in declarations()[name][1]]
