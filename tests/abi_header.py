"""Checker side of the C boundaries: what a header of include/ declares (prototypes, integer #defines) and what the library exports, read
once for tests/test_abi.py (include/dbw_hip.h) and tests/test_abi_families.py (every add-on header of dbw_amd/_lib.FAMILIES)."""
import ctypes
import os
import re
import subprocess

from dbw_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')
CTYPE = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t,
         'dbw_stream_t': ctypes.c_void_p}


def text(header):
    return open(os.path.join(INCLUDE, header)).read()


def prototypes(header):
    """{name: (return type as written, [ctypes of the arguments])} of every dbw_* function include/<header> declares; any pointer is a
    c_void_p, an argument of a type outside CTYPE is a KeyError."""
    src = re.sub(r'/\*.*?\*/', '', text(header), flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r'\b(int64_t|int|size_t|void \*|void|const char \*|dbw_step_plan \*)\s*(dbw_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S):
        args = ' '.join(args.split())
        protos[name] = (ret.strip(), [] if args in ('', 'void') else [ctypes.c_void_p if '*' in a else CTYPE[a.replace('const ', '').split()[0]]
                                                                      for a in args.split(',')])
    return protos


def defines(header):
    """{macro: value} of the integer #defines of include/<header>."""
    return {name: int(value) for name, value in re.findall(r'^#define (\w+) \(?(-?\d+)\)?', text(header), flags=re.M)}


def exported():
    """The dbw_* functions libdbw_hip.so defines, by nm."""
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r' T (dbw_\w+)', syms))
