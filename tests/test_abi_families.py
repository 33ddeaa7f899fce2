"""CPU: every add-on C boundary of dbw_amd/_lib.FAMILIES (a header beside include/dbw_hip.h) against its ctypes binding and the library,
one parametrised id per family, and _lib.family() on a stand-in library.  A new family is a row of FAMILIES and a row of CHECKS here."""
import ctypes
import os
import re
import subprocess
import types

import pytest

import abi_header as AH
from dbw_amd import _lib

# what the table of _lib.py cannot say about itself: the revision pinned as a literal, the Python constants that mirror a #define (FOO of
# _lib is DBW_FOO of the header), `symbols`: a dbw_* function the library exports whose name contains one of these belongs to the family,
# `text`: words that neither include/dbw_hip.h nor the header of a family listed before this one contains
CHECKS = {
    'eval': dict(version=1, constants=(), symbols=('eval', 'nn_points', 'lattice', 'downsample'),
                 text=('dbw_eval', 'nn_points', 'lattice', 'downsample')),
    'viz': dict(version=1, constants=(), symbols=('viz', 'render_lit', 'vertex_normals'), text=('dbw_viz', 'render_lit', 'vertex_normals')),
    'export': dict(version=1, constants=('FRAME_HWC', 'FRAME_EDGE_FIRST', 'FRAME_CLAMP_INPUT'), symbols=('export', 'frames'),
                   text=('dbw_export', 'frames_u8')),
    'ingest': dict(version=1, constants=('RESAMPLE_AUTO', 'RESAMPLE_GENERAL', 'RESAMPLE_FUSED'), symbols=('resample', 'ingest'),
                   text=('dbw_ingest', 'resample')),
    'lens': dict(version=1, constants=('LENS_N_PARAMS',), symbols=('lens', 'undistort'), text=('dbw_lens', 'undistort')),
    'monitor': dict(version=1, constants=('METER_MAX_VALUES',), symbols=('monitor', 'meter', 'scores'),
                    text=('dbw_monitor', 'dbw_meter', 'image_scores')),
    'icp': dict(version=1, constants=('ICP_TRACE_PER_INSTANCE',), symbols=('icp',), text=('dbw_icp',)),
}
NAMES = list(_lib.FAMILIES)


def _names(f):
    return set(f.signatures) | set(f.other_signatures) | {f.version_fn}


def test_every_header_beside_dbw_hip_is_a_family():
    assert set(CHECKS) == set(NAMES)
    assert sorted(f.header for f in _lib.FAMILIES.values()) == sorted(h for h in os.listdir(AH.INCLUDE) if h != 'dbw_hip.h')
    lib = _lib.load()
    assert lib.dbw_abi_version() == _lib.ABI_VERSION == AH.defines('dbw_hip.h')['DBW_ABI_VERSION'] == 7


@pytest.mark.parametrize('name', NAMES)
def test_header_is_plain_c99(name, tmp_path):
    """The header alone compiles as C99 with warnings as errors, and the program's main finds the revision and the mirrored constants."""
    f, c = _lib.FAMILIES[name], CHECKS[name]
    conds = [f'{f.macro} == {c["version"]}'] + [f'DBW_{k} == {getattr(_lib, k)}' for k in c['constants']]
    src = tmp_path / f'{name}.c'
    src.write_text(f'#include "{f.header}"\nint main(void) {{ return {" && ".join(conds)} ? 0 : 1; }}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', AH.INCLUDE, str(src), '-o', str(tmp_path / name)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert subprocess.run([str(tmp_path / name)]).returncode == 0, conds


@pytest.mark.parametrize('name', NAMES)
def test_header_matches_the_binding_and_the_library(name):
    f, c = _lib.FAMILIES[name], CHECKS[name]
    protos = AH.prototypes(f.header)
    assert {ret for ret, _ in protos.values()} <= {'int', 'size_t'}
    ints = {n: types_ for n, (ret, types_) in protos.items() if ret == 'int'}
    sizes = {n: types_ for n, (ret, types_) in protos.items() if ret == 'size_t'}
    assert set(ints) == set(f.signatures) | {f.version_fn} and set(sizes) == set(f.other_signatures)
    lib = _lib.load()
    for n, types_ in f.signatures.items():
        assert ints[n] == types_, n
        assert getattr(lib, n).argtypes == types_ and getattr(lib, n).restype == ctypes.c_int, n
    for n, (restype, types_) in f.other_signatures.items():
        assert sizes[n] == types_ and restype == ctypes.c_size_t, n
        assert getattr(lib, n).argtypes == types_ and getattr(lib, n).restype == restype, n
    defs = AH.defines(f.header)
    assert getattr(lib, f.version_fn)() == getattr(_lib, f'{name.upper()}_ABI_VERSION') == defs[f.macro] == c['version']
    assert _lib.family(name) is lib
    for k in c['constants']:
        assert getattr(_lib, k) == defs[f'DBW_{k}'], k
    # the library exports every name, and no other function that reads like one of this family
    mine, exported = _names(f), AH.exported()
    assert mine <= exported and {n for n in exported if any(w in n for w in c['symbols'])} == mine
    # no name is bound twice: not in the tables of include/dbw_hip.h, not in another family's, and none reads like another family's
    assert not mine & (set(_lib.SIGNATURES) | set(_lib.OTHER_SIGNATURES))
    for other in NAMES:
        if other != name:
            assert not mine & _names(_lib.FAMILIES[other]), other
            assert not any(w in n for n in mine for w in CHECKS[other]['symbols']), other
    # include/dbw_hip.h and the headers of the families before this one do not speak of it
    for h in ['dbw_hip.h'] + [_lib.FAMILIES[o].header for o in NAMES[:NAMES.index(name)]]:
        text = AH.text(h)
        assert not any(w in text for w in mine | set(c['text'])), h


@pytest.mark.parametrize('name', NAMES)
def test_family_refuses_a_library_without_it(name, monkeypatch):
    monkeypatch.setattr(_lib, '_lib', types.SimpleNamespace())               # load() hands out its cache: no library, no GPU
    with pytest.raises(RuntimeError, match=re.escape(f'(include/{_lib.FAMILIES[name].header}): rebuild it')):
        _lib.family(name)


@pytest.mark.parametrize('name', NAMES)
def test_family_refuses_a_library_of_another_revision(name, monkeypatch):
    f = _lib.FAMILIES[name]
    want = AH.defines(f.header)[f.macro]
    stub = types.SimpleNamespace(**{f.version_fn: lambda: want + 1})
    monkeypatch.setattr(_lib, '_lib', stub)
    with pytest.raises(RuntimeError, match=re.escape(f'ABI {want + 1}, include/{f.header} declares {want}: rebuild it')):
        _lib.family(name)
    setattr(stub, f.version_fn, lambda: want)
    assert _lib.family(name) is stub
